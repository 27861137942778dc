"""The update workspace keeps its size: csrc/tma_workspace.h is the one definition of where every region lives, the Python side allocates
what tma_ppo_workspace_bytes says and the persistent kernels address the regions by the same offsets -- so the total of every layout class
is pinned here.  Host-only: the query launches nothing."""
import ctypes as C

import pytest

F32, BF16, BF16X3 = 0, 1, 2

# (obs_dim, hidden, act_dim, continuous, mfma_dtype) -> bytes.  The values are what the library returned at commit e730067 (ABI 217, the last
# one whose drivers added the region sizes up by hand), queried from a build of that commit; one shape per layout class.
EXPECTED = [
    ((4, 64, 5, 0, F32), 22209120),  # H = 64 images, fold state
    ((9, 64, 7, 0, F32), 22612576),  # H = 64, no packed records
    ((6, 256, 5, 0, F32), 106444640),  # h256p layout: f32 fragments + the persistent launch's snapshot
    ((21, 256, 3, 0, F32), 111116848),  # f32 fragments
    ((172, 256, 20, 1, F32), 698549888),  # f32 two-pass dz1 cache
    ((105, 256, 8, 1, F32), 674613888),  # f32 two-pass dz1 cache (seven k-tiles)
    ((4, 128, 5, 0, F32), 39759616),  # wide f32, H = 128
    ((6, 256, 5, 0, BF16), 104804096),  # bf16 single pass
    ((48, 128, 4, 0, BF16), 181103744),  # bf16 two-pass cache
    ((172, 256, 20, 1, BF16), 430114432),  # bf16 two-pass cache
    ((6, 256, 5, 0, BF16X3), 106444640),  # bf16x3 split
    ((300, 512, 4, 0, F32), 445393408),  # generic kernel
]
HEADER_BYTES = 139264  # the fixed header alone: what a null or invalid `dims` gets


@pytest.mark.parametrize("shape,expected", EXPECTED, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_workspace_bytes_of_every_layout_class(shape, expected):
    import torch

    from three_mlagents_amd import _lib

    assert _lib.lib().tma_ppo_workspace_bytes(C.byref(_lib.PolicyDims(*shape, -1))) == expected
    assert not torch.cuda.is_initialized()


def test_workspace_bytes_without_a_valid_shape_is_the_header():
    from three_mlagents_amd import _lib

    assert _lib.lib().tma_ppo_workspace_bytes(None) == HEADER_BYTES
    assert _lib.lib().tma_ppo_workspace_bytes(C.byref(_lib.PolicyDims(4, 65, 5, 0, F32, -1))) == HEADER_BYTES  # hidden no multiple of 64
    assert _lib.lib().tma_ppo_workspace_bytes(C.byref(_lib.PolicyDims(6, 128, 5, 0, BF16X3, -1))) == HEADER_BYTES  # the split is 256-wide only
