"""GPU: `op._dispatch.native` on the real library — one launch, and one call the library refuses before launching."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_one_launch_through_the_launcher():
    from stylerenderer_amd.op._dispatch import native

    g = torch.Generator(DEV).manual_seed(1)
    a = torch.randn(2, 64, device=DEV, generator=g)
    b = torch.randn(2, 64, device=DEV, generator=g)
    out = torch.empty((), device=DEV)
    assert native(a).sr_mse_fwd(out, a, b, a.numel()) is None
    want = torch.mean((a.double() - b.double()) ** 2)
    torch.testing.assert_close(out.double(), want, rtol=2e-6, atol=0)


def test_a_refused_call_raises_under_the_called_name():
    """A 5x5 weight gradient is no geometry of the plan: SR_EINVAL before anything is launched."""
    from stylerenderer_amd.op._dispatch import native

    x = torch.zeros(1, 4, 8, 8, device=DEV)
    gy = torch.zeros(1, 4, 8, 8, device=DEV)
    dwt = torch.zeros(25, 4, 4, device=DEV)
    scratch = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match="sr_conv2d_wgrad_mfma failed"):
        native(x).sr_conv2d_wgrad_mfma(dwt, x, gy, None, None, 1, 4, 4, 8, 8, 8, 8, 5, 1, 2, 0, scratch)
    torch.cuda.synchronize()
    assert not dwt.any()
