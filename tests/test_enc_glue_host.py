"""The form of the BatchNorm apply pass that also writes the 2x2 max-pool (include/uaps_hip.h: uaps_bn_apply_pool_support), held on
the host: H even, W a multiple of 8, 2 W dividing the 4096-float chunk -- and every encoder level of the 256 x 256 and 512 x 512
configurations inside it.  Needs the built library, no GPU."""
import pytest

ENOFORM = -4


def _support():
    from uaps_amd import _lib
    return _lib.lib().uaps_bn_apply_pool_support


def test_the_support_function_is_the_stated_condition():
    f = _support()
    for H in range(2, 1025):
        for W in range(2, 1025):
            want = H % 2 == 0 and W % 8 == 0 and 4096 % (2 * W) == 0
            assert (f(H, W) == 0) == want, (H, W)
            if not want:
                assert f(H, W) == ENOFORM, (H, W)


@pytest.mark.parametrize("side", [256, 512])
def test_every_pooled_encoder_level_is_inside_the_form(side):
    f = _support()
    for level in range(4):                 # levels 0..3 are pooled; the fifth feeds the decoders only
        s = side >> level
        assert f(s, s) == 0, s
    for s in (16, 32, 64, 128, 256):
        assert f(s, s) == 0, s


def test_degenerate_sizes_are_refused():
    f = _support()
    for H, W in ((0, 8), (-2, 8), (2, 0), (2, -8), (4, 12), (3, 8), (8, 4), (2, 4096)):
        assert f(H, W) == ENOFORM, (H, W)
