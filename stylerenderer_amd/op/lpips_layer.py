"""One LPIPS layer — normalize_tensor, squared difference, `lin` 1x1 convolution, spatial average — as one fused forward
and one fused backward launch (C ABI sr_lpips_layer_fwd / _bwd, csrc/lpips.hip) instead of ~25 ATen launches.

    lpips_layer(f0 [B, C, H, W], t_normalised [B | 1, C, H, W], lin [1, C, 1, 1] | [C]) -> [B, 1, 1, 1]

Differentiable once, with respect to f0 (the latent-inversion loop optimises the image behind f0; the target and the
learned heads are fixed).  reference lpips/networks_basic.py:62-85, lpips/__init__.py:42-44.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from ._dispatch import native, require_f32

EPS = 1e-10


def supported(f0, t, lin):
    return (f0.device.type == "cuda" and f0.dtype == torch.float32 and f0.dim() == 4 and t.dtype == torch.float32
            and t.shape[1:] == f0.shape[1:] and t.shape[0] in (1, f0.shape[0]) and lin.numel() == f0.shape[1]
            and not t.requires_grad and not lin.requires_grad)


SLICES = 16                      # csrc/lpips.hip SL: channel c is summed in slice c % 16, at step c // 16


def normalize_in_kernel_order(f, eps=EPS):
    """f / (sqrt(sum_c f^2) + eps) of f [B, C, H, W] with the channel sum taken in k_lpips_fwd's order: 16 interleaved
    slices, each from 0 in ascending channel order, then the slices from 0 in order.  Each step is one rounded float
    operation here as there (the file is compiled without contraction), so this is the normalisation the layer kernel
    applies to its f0: lpips_layer(f, normalize_in_kernel_order(f), lin) is exactly 0 with a zero gradient, which
    torch's own sum over the channels (another order, a last-bit difference in places) does not give.  Once per target,
    not per step: plain element-wise launches."""
    b, c, h, w = f.shape
    sq = f * f
    pad = (-c) % SLICES
    if pad:                                           # (x + 0 = x: short slices are summed as the kernel sums them)
        sq = torch.cat((sq, sq.new_zeros(b, pad, h, w)), 1)
    sq = sq.view(b, -1, SLICES, h, w)
    ss = torch.zeros_like(sq[:, 0])
    for k in range(sq.shape[1]):
        ss = ss + sq[:, k]
    tot = torch.zeros_like(ss[:, 0])
    for i in range(SLICES):
        tot = tot + ss[:, i]
    return f / (torch.sqrt(tot) + eps).unsqueeze(1)


class _LpipsLayer(Function):
    @staticmethod
    def forward(ctx, f0, t, lin):
        require_f32(f0, "lpips_layer")
        f0 = f0.contiguous()
        t = t.contiguous()
        lin = lin.reshape(-1).contiguous()
        b, c, h, w = f0.shape
        hw = h * w
        d = torch.empty(b, dtype=f0.dtype, device=f0.device)
        scratch = torch.empty(_lib.lib().sr_lpips_layer_scratch_floats(b, hw), dtype=f0.dtype, device=f0.device)
        ctx.bstride = c * hw if t.shape[0] == b else 0            # (one target for the whole batch: stride 0)
        native(f0).sr_lpips_layer_fwd(d, f0, t, lin, b, c, hw, ctx.bstride, EPS, scratch)
        ctx.save_for_backward(f0, t, lin)
        return d.view(b, 1, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, gd):
        f0, t, lin = ctx.saved_tensors
        b, c, h, w = f0.shape
        gd = gd.reshape(b).contiguous()
        gf = torch.empty_like(f0)
        native(f0).sr_lpips_layer_bwd(gf, gd, f0, t, lin, b, c, h * w, ctx.bstride, EPS)
        return gf, None, None


def lpips_layer(f0, t_normalised, lin):
    return _LpipsLayer.apply(f0, t_normalised, lin)


class _MSE(Function):
    """mean((a - b)^2) -> 0-d, differentiable once w.r.t. a (sr_mse_fwd / _bwd: one launch each way)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty((), dtype=a.dtype, device=a.device)
        native(a).sr_mse_fwd(out, a, b, a.numel())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a)
        native(a).sr_mse_bwd(ga, g.contiguous(), a, b, a.numel())
        return ga, None


def mse(a, b):
    """torch.mean((a - b) ** 2) with b fixed; device float32 tensors take the fused kernels."""
    if (a.device.type == "cuda" and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape
            and a.numel() > 0 and not b.requires_grad and a.contiguous().data_ptr() % 16 == 0
            and b.contiguous().data_ptr() % 16 == 0):
        return _MSE.apply(a, b)
    return torch.mean((a - b) ** 2)


class _MaxPool2(Function):
    """F.max_pool2d(x, 2, 2) on even maps — sr_maxpool2_fwd / _bwd (the arg-max is recomputed from the saved input)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        b, c, h, w = x.shape
        out = torch.empty((b, c, h // 2, w // 2), dtype=x.dtype, device=x.device)
        native(x).sr_maxpool2_fwd(out, x, b * c, h, w)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        b, c, h, w = x.shape
        gx = torch.empty_like(x)
        native(x).sr_maxpool2_bwd(gx, g.contiguous(), x, b * c, h, w)
        return gx


def max_pool2(x):
    """2 x 2 / stride 2 max pooling; device float32 tensors with even maps take the library's kernels."""
    if (x.device.type == "cuda" and x.dtype == torch.float32 and x.dim() == 4 and x.shape[2] % 2 == 0
            and x.shape[3] % 2 == 0 and x.numel() > 0):
        return _MaxPool2.apply(x)
    return torch.nn.functional.max_pool2d(x, 2, 2)


# ---- per-sample terms of the batched inversion loss ------------------------------------------------------------------
class _MSERows(Function):
    """out[b] = mean((a[b] - t[b])^2) over row b of a [B, ...] -> [B], differentiable once w.r.t. a (sr_mse_rows_fwd:
    chunk partials and a fixed-order finish; sr_mse_rows_bwd: one launch)."""

    @staticmethod
    def forward(ctx, a, t):
        a, t = a.contiguous(), t.contiguous()
        b = a.shape[0]
        n = a.numel() // b
        out = torch.empty(b, dtype=a.dtype, device=a.device)
        scratch = torch.empty(_lib.lib().sr_mse_rows_scratch_floats(b, n), dtype=a.dtype, device=a.device)
        native(a).sr_mse_rows_fwd(out, a, t, b, n, scratch)
        ctx.save_for_backward(a, t)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, t = ctx.saved_tensors
        b = a.shape[0]
        ga = torch.empty_like(a)
        native(a).sr_mse_rows_bwd(ga, g.contiguous(), a, t, b, a.numel() // b)
        return ga, None


def mse_rows(a, t):
    """((a - t) ** 2) averaged over everything but the first dimension -> [B], t fixed; device float32 tensors take
    the kernels (`mse` is the batch-wide mean)."""
    if (a.device.type == "cuda" and a.dtype == torch.float32 and t.dtype == torch.float32 and a.shape == t.shape
            and a.dim() >= 1 and a.numel() > 0 and not t.requires_grad):
        return _MSERows.apply(a, t)
    return ((a - t) ** 2).reshape(a.shape[0], -1).mean(1)


class _FitLossRows(Function):
    """(rows [B], total []) of `fit_loss_rows` in one launch; the backward is one launch that writes the gradient of
    every layer distance and of the pixel term, and hands `reg` the total's gradient.  `rows` is not differentiable."""

    @staticmethod
    def forward(ctx, pixel_weight, coeff, sigma, shape_reg, mse, reg, *layers):
        ctx.set_materialize_grads(False)
        b = mse.shape[0]
        rows = torch.empty(b, dtype=mse.dtype, device=mse.device)
        total = torch.empty((), dtype=mse.dtype, device=mse.device)
        d = [t.reshape(b).contiguous() for t in layers]
        m = mse.contiguous()
        c = coeff.detach().contiguous() if coeff is not None else None
        s = sigma.detach().contiguous() if sigma is not None else None
        native(m).sr_fit_loss_rows(rows, total, *d, m, float(pixel_weight), c, s, float(shape_reg), b,
                                   c.shape[1] if c is not None else 0)
        ctx.mark_non_differentiable(rows)
        ctx.pixel_weight = float(pixel_weight)
        ctx.layer_shapes = [t.shape for t in layers]
        ctx.has_reg = reg is not None
        return rows, total

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rows, g_total):
        n_in = 6 + len(ctx.layer_shapes)
        if g_total is None:
            return (None,) * n_in
        b = ctx.layer_shapes[0][0]
        gd = torch.empty(b, dtype=g_total.dtype, device=g_total.device)
        gm = torch.empty_like(gd)
        native(gd).sr_fit_loss_rows_bwd(gd, gm, g_total.contiguous(), ctx.pixel_weight, b)
        greg = g_total if ctx.has_reg else None
        return (None, None, None, None, gm, greg) + tuple(gd.view(s) for s in ctx.layer_shapes)


def fit_loss_rows(layers, mse, pixel_weight, coeff=None, sigma=None, shape_reg=0.0, reg=None, prior_rows=None):
    """Per-sample losses of a batched fit and their sum:

        rows[b] = sum_k layers[k][b] + pixel_weight * mse[b] (+ shape_reg * sum_j (coeff[b, j] / sigma[j])^2)
        total   = sum_b rows[b]

    layers: the five LPIPS layer distances ([B] or [B, 1, 1, 1] each), mse [B] (`mse_rows`), coeff [B, d] with the
    prior.  Returns (rows [B], not differentiable, total []).  On the device the prior's gradient is NOT formed here:
    `reg`, the scalar shape_reg * regulation(coeff) of op.morph.morph_mesh, receives d(total)/d(reg) and the morph node
    carries it to the coefficients (reg is required with coeff).  The composite (CPU, float64) differentiates the prior
    through coeff and does not use reg.

    A prior that is not a diagonal Gaussian (op.blend's Dirichlet / Beta) comes as `prior_rows` [B], every sample's own
    prior value (not differentiable), with `reg` their differentiable sum and no coeff: rows[b] += prior_rows[b],
    total += reg, on every device."""
    if len(layers) != 5:
        raise ValueError("fit_loss_rows: five LPIPS layer distances expected, got %d" % len(layers))
    if prior_rows is not None:
        if coeff is not None or reg is None:
            raise ValueError("fit_loss_rows: prior_rows comes with reg and without coeff")
        rows, total = fit_loss_rows(layers, mse, pixel_weight)
        return rows + prior_rows.detach().to(rows.dtype), total + reg
    ts = list(layers) + [mse] + ([coeff] if coeff is not None else [])
    if all(t.device.type == "cuda" and t.dtype == torch.float32 for t in ts):
        if coeff is not None and reg is None:
            raise ValueError("fit_loss_rows: the device node needs the morph node's reg with coeff")
        return _FitLossRows.apply(float(pixel_weight), coeff, sigma, float(shape_reg), mse, reg, *layers)
    b = mse.shape[0]
    rows = layers[0].reshape(b)
    for t in layers[1:]:
        rows = rows + t.reshape(b)
    rows = rows + pixel_weight * mse
    if coeff is not None:
        x = coeff / sigma.view(1, -1) if sigma is not None else coeff
        rows = rows + shape_reg * (x ** 2).sum(1)
    return rows.detach(), rows.sum()
