"""CPU: `ofx_raft_workspace_bytes_mode` sizes the layout a call's flags actually carve -- the volume-free mode (OFX_RAFT_ALT_CORR)
drops the correlation pyramid from the workspace.  The library loads without a device; no GPU work is issued."""
import pytest

ALT, SH2, SH1 = 8, 2, 4


def _lib_():
    from sd_animation_optical_flow_amd import _lib
    return _lib.lib()


def _pyramid_bytes(B, H, W):
    N = (H // 8) * (W // 8)
    return 4 * B * N * N * (1 + 1 / 4 + 1 / 16 + 1 / 64)


def test_mode_size_without_flags_is_the_classic_size():
    lib = _lib_()
    B, H, W = 64, 768, 512
    assert lib.ofx_raft_workspace_bytes_mode(None, 0, B, H, W, 0) == lib.ofx_raft_workspace_bytes(None, B, H, W) > 0
    assert lib.ofx_raft_workspace_bytes_mode(None, 2 * B, B, H, W, 0) == lib.ofx_raft_workspace_bytes_pairs(None, 2 * B, B, H, W) > 0


@pytest.mark.parametrize("n_images", [0, 65, 128])
def test_volume_free_layout_has_no_pyramid(n_images):
    lib = _lib_()
    B, H, W = 64, 768, 512
    vol = lib.ofx_raft_workspace_bytes_mode(None, n_images, B, H, W, 0)
    alt = lib.ofx_raft_workspace_bytes_mode(None, n_images, B, H, W, ALT)
    print(f"n_images={n_images}: volume layout {vol / 1e9:.2f} GB, volume-free {alt / 1e9:.2f} GB, pyramid {_pyramid_bytes(B, H, W) / 1e9:.2f} GB")
    assert 0 < alt < vol - 0.9 * _pyramid_bytes(B, H, W)
    # flags that do not change the layout do not change the size (BGR, warm start, serial)
    assert lib.ofx_raft_workspace_bytes_mode(None, n_images, B, H, W, ALT | 1 | 32 | 2048) == alt


def test_shared_key_frame_layouts_are_no_larger():
    lib = _lib_()
    B, H, W = 16, 1088, 1920
    alt = lib.ofx_raft_workspace_bytes_mode(None, 0, B, H, W, ALT)
    assert 0 < lib.ofx_raft_workspace_bytes_mode(None, 0, B, H, W, ALT | SH2) < alt
    assert 0 < lib.ofx_raft_workspace_bytes_mode(None, 0, B, H, W, ALT | SH1) < alt
    assert alt < lib.ofx_raft_workspace_bytes(None, B, H, W) - 0.9 * _pyramid_bytes(B, H, W)       # 16 pairs at 1080p: a 90 GB pyramid


def test_bad_arguments_return_zero():
    lib = _lib_()
    f = lib.ofx_raft_workspace_bytes_mode
    assert f(None, 0, 0, 512, 768, ALT) == 0            # no pairs
    assert f(None, 0, -1, 512, 768, 0) == 0
    assert f(None, 0, 1, 100, 96, ALT) == 0             # H not a multiple of 8
    assert f(None, 0, 1, 96, 100, ALT) == 0
    assert f(None, 0, 1, 0, 96, 0) == 0
    assert f(None, -1, 1, 512, 768, ALT) == 0           # negative image count
    assert f(None, 0, 1, 512, 768, -1) == 0             # flags that are no flags
    assert f(None, 0, 1, 512, 768, 1 << 20) == 0
    assert f(None, 4, 2, 512, 768, ALT | SH2) == 0      # the indexed-pairs entry points take no shared-image flag
    assert f(None, 4, 2, 512, 768, SH1) == 0
