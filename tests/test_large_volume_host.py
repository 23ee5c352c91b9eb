"""Volumes above 2^30 voxels at the C ABI, without a GPU (the argument checks run before any
launch, tests/test_abi.py::test_argument_checks_return_errors_without_touching_a_device).

Every entry is called with non-null dummy pointers and B = -1: an entry that takes the volume gets
past the size check and fails on the batch check; an entry that keeps 32-bit offsets fails on the
size check, naming itself and the 2^30 cap; every entry refuses dims above the new cap."""
import ctypes

import pytest

from diffdrr_amd import _lib

# entry -> (index of dx, index of B); dy, dz follow dx
EXTENDED = {
    "ddrr_siddon_forward": (1, 8),
    "ddrr_siddon_forward_bricks": (1, 7),
    "ddrr_siddon_forward_bricks_masked": (1, 7),
    "ddrr_siddon_backward_volume_bricks": (0, 7),
    "ddrr_siddon_backward_volume": (1, 9),
    "ddrr_siddon_backward_midpoint": (1, 9),
    "ddrr_trilinear_forward": (1, 8),
    "ddrr_trilinear_forward_bricks": (1, 7),
    "ddrr_trilinear_backward_volume_bricks": (0, 7),
    "ddrr_trilinear_backward": (1, 9),
    "ddrr_trilinear_backward_max": (1, 9),
}
CAPPED = {
    "ddrr_siddon_forward_channels": (2, 9),
    "ddrr_siddon_backward_channels": (2, 10),
    "ddrr_siddon_forward_channels_bricks": (2, 8),
    "ddrr_siddon_forward_channels_bricks_words": (1, 7),
    "ddrr_siddon_backward_channels_bricks": (2, 8),
    "ddrr_siddon_backward_channels_volume_bricks": (1, 8),
    "ddrr_trilinear_forward_channels": (2, 9),
    "ddrr_trilinear_backward_channels": (2, 10),
    "ddrr_trilinear_forward_channels_bricks": (2, 8),
    "ddrr_trilinear_backward_channels_bricks": (2, 8),
    "ddrr_trilinear_backward_channels_volume_bricks": (1, 8),
    "ddrr_siddon_segments": (1, 8),
    "ddrr_siddon_segments_backward": (1, 9),
    "ddrr_trilinear_samples": (1, 8),
    "ddrr_trilinear_samples_backward": (1, 9),
    "ddrr_siddon_forward_f64": (1, 8),
    "ddrr_siddon_backward_f64": (0, 9),
    "ddrr_trilinear_forward_f64": (1, 8),
    "ddrr_trilinear_backward_f64": (1, 9),
    "ddrr_siddon_segments_general": (2, 9),
    "ddrr_siddon_segments_general_backward": (2, 10),
    "ddrr_trilinear_samples_general": (2, 9),
    "ddrr_trilinear_samples_general_backward": (2, 10),
}

SHAPE_A = (1024, 1024, 1040)  # 1.09e9 voxels: above 2^30
SHAPE_B = (1280, 1280, 1312)  # 2.15e9 voxels: above 2^31
SHAPE_MAX = (16384, 1024, 1024)  # 2^34 voxels exactly: the cap
ABOVE_CAP = [
    (16385, 1024, 1024),  # > 2^34 voxels
    (1 << 16, 1 << 14, 2),  # a dim of 2^16 (2^31 voxels)
    (8, 1 << 14, (1 << 14) + 1),  # dy * dz > 2^28 (2^31 voxels)
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build_hip()
    return _lib.DdrrLibrary(_lib.LIB_PATH)


def _call(lib, name, dims, dims_at, b_at, B):
    """`name` with dummy arguments: every pointer non-null, every int 1, dims and B as given."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = getattr(lib.cdll, name)
    args = []
    for t in fn.argtypes:
        args.append({ctypes.c_void_p: p, ctypes.c_int: 1, ctypes.c_long: 1}.get(t, 0.5))
    for k in range(3):
        assert fn.argtypes[dims_at + k] is ctypes.c_int
        args[dims_at + k] = dims[k]
    assert fn.argtypes[b_at] is ctypes.c_int
    args[b_at] = B
    rc = fn(*args)
    return rc, lib.cdll.ddrr_last_error().decode()


def test_tables_cover_the_abi():
    """Every entry of include/diffdrr_hip.h that takes volume dims is in one of the two tables."""
    import os
    import re

    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "diffdrr_hip.h")).read()
    takes_dims = {m.group(1) for m in re.finditer(r"\b(?:int|long) (ddrr_\w+)\(([^;]*?)\);", header, re.S)
                  if re.search(r"\bint dx,\s*int dy,\s*int dz\b", m.group(2))}
    # sizes, or the rays alone (no volume is read)
    takes_dims -= {"ddrr_brick_workspace_bytes", "ddrr_brick_launch_workspace_bytes",
                   "ddrr_trilinear_alpha_range"}
    assert len(takes_dims) > 30
    assert takes_dims == set(EXTENDED) | set(CAPPED)


@pytest.mark.parametrize("shape", [SHAPE_A, SHAPE_B, SHAPE_MAX])
@pytest.mark.parametrize("name", sorted(EXTENDED))
def test_extended_entries_take_volumes_above_2_30_voxels(lib, name, shape):
    rc, err = _call(lib, name, shape, *EXTENDED[name], B=-1)
    assert rc != 0 and "negative batch" in err, err


@pytest.mark.parametrize("name", sorted(CAPPED))
def test_capped_entries_refuse_volumes_above_2_30_voxels(lib, name):
    rc, err = _call(lib, name, SHAPE_A, *CAPPED[name], B=-1)
    assert rc != 0 and "2^30" in err, err
    route = err.split(" takes ")[0]
    assert name in route or ("f64" in name and "float64" in route) or \
        ("general" in name and "general path" in route), err
    # at 2^30 voxels exactly, the size check passes as before
    rc, err = _call(lib, name, (1024, 1024, 1024), *CAPPED[name], B=-1)
    assert rc != 0 and "negative batch" in err, err


@pytest.mark.parametrize("shape", ABOVE_CAP)
@pytest.mark.parametrize("name", sorted(EXTENDED))
def test_every_entry_refuses_volumes_above_the_cap(lib, name, shape):
    rc, err = _call(lib, name, shape, *EXTENDED[name], B=-1)
    assert rc != 0 and "2^34" in err, err


def test_small_volumes_are_checked_as_before(lib):
    """Up to 2^30 voxels no new limit applies: a 2^30-voxel slab of any shape still gets through."""
    for shape in [(1, 1 << 15, 1 << 15), (1 << 30, 1, 1), (4, 4, 4)]:
        rc, err = _call(lib, "ddrr_siddon_forward", shape, *EXTENDED["ddrr_siddon_forward"], B=-1)
        assert rc != 0 and "negative batch" in err, err


def test_brick_workspaces_hold_at_the_cap(lib):
    """The workspace sizes of the largest supported volume are exact 64-bit products."""
    q = lib.query
    dx, dy, dz = SHAPE_MAX
    n32 = -(-dx // 32) * -(-dy // 32) * -(-dz // 32)
    assert q("ddrr_brick_launch_workspace_bytes", dx, dy, dz) == 256 + (n32 * 8 + 255) // 256 * 256
    packed = q("ddrr_brick_workspace_bytes", dx, dy, dz, _lib.BRICKS_Q16_PACKED)
    ranges = q("ddrr_brick_workspace_bytes", dx, dy, dz, _lib.BRICKS_Q16)
    # +52 % of the volume's fp32 bytes for the packed bricks, as at 512^3
    assert 0.5 < (packed - ranges) / (4 * dx * dy * dz) < 0.55
    assert ranges > 12 * n32
