"""The shared identity of a multi-view fit (csrc/share.hip).

A batched LatentInverter with shared_identity=K fits B views of one subject: the leading K columns of coeff [B, d] are one
variable theta [K] that every row holds a copy of.  The objective is sum_b L_b, so d/d theta = sum_b dL_b / d coeff[b, :K]:
between backward and the optimiser's step the leading K columns of every row of coeff.grad are replaced by their sum over
the rows.  Rows that start equal then see the same gradient and the same element-wise Adam and stay equal bit for bit.

  share_rows_(g, k)   in place on g [B, d], contiguous:  s[j] = ((g[0, j] + g[1, j]) + g[2, j]) + ...  in row order, in g's
                      float type; then g[b, j] = s[j] for every b and every j < k.  Columns >= k are not touched.

CPU tensors and float64 run the torch loop below, which is the definition.  Float32 device tensors run sr_share_rows: one
launch, one lane per column, nothing allocated and nothing read back, so the call can be captured; the additions are the
definition's in its order, so the result is the host's bit for bit.  Under SR_STRICT_NATIVE=1 a device tensor the kernel
does not take (float64) raises.
"""
import torch

from ._dispatch import is_device_tensor, native, strict_native


def share_rows_host_(g, k):
    """The definition: B - 1 additions per column, in row order."""
    s = g[0, :k].clone()
    for b in range(1, g.shape[0]):
        s = s + g[b, :k]
    g[:, :k] = s
    return g


@torch.no_grad()
def share_rows_(g, k):
    """Replaces the leading k columns of every row of g [B, d] (contiguous, floating point) by their sum over the rows, in
    place; returns g."""
    if g.dim() != 2 or not g.is_floating_point():
        raise ValueError("share_rows_: g must be a floating-point [B, d], got %s %s" % (g.dtype, tuple(g.shape)))
    if not g.is_contiguous():
        raise ValueError("share_rows_: g must be contiguous")
    b, d = int(g.shape[0]), int(g.shape[1])
    k = int(k)
    if b < 1 or not 1 <= k <= d:
        raise ValueError("share_rows_: needs B >= 1 and 1 <= k <= d, got B = %d, d = %d, k = %d" % (b, d, k))
    if not (is_device_tensor(g) and g.dtype == torch.float32):
        if is_device_tensor(g) and strict_native():
            raise RuntimeError("share_rows_: SR_STRICT_NATIVE=1 and the kernel takes float32 device tensors only")
        return share_rows_host_(g, k)
    native(g).sr_share_rows(g, b, d, k)
    return g
