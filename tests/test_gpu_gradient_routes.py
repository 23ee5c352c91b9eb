"""The route matrix and the layout invariance of tests/test_gradient_routes.py on the MI355X.

The route matrix runs at a size where the brick grid matters: a CT-like 192 x 192 x 67 volume (several
bricks per axis, ragged edges), a 112 x 96 detector, 3 poses; ``patch_size`` 44 -> 5 chunks of 2151 /
2148 rays (no chunk ends on a detector row), a 10 % subsample -> 1075 rays, with patches 5 chunks of
215.  Every case records the C-ABI entries it took (the masked brick kernel, the per-ray kernels, ...).

Layout invariance on the device allows only the reordering of float atomics (1e-5 of the largest
value), except where the path is bit-reproducible: the fixed-point brick volume gradient of a Siddon
sum (csrc/bricks.hip LdsAbsAddT).  Its scale is taken from a sum of one float bound per pose, added
by atomics; with two poses that sum does not depend on their order, so those cases use B = 2."""
import pytest
import torch

from diffdrr_amd import ops
from diffdrr_amd.data import make_subject, phantom_volume

import test_gradient_routes as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    dims = (192, 192, 67)
    vol = phantom_volume(dims, seed=4)
    g = torch.Generator().manual_seed(9)
    B = 3
    rot = (torch.rand(B, 3, generator=g) - 0.5) * 1.2
    xyz = torch.tensor([0.0, 500.0, 0.0]) + (torch.rand(B, 3, generator=g) - 0.5) * 30
    return dict(
        subject=make_subject(vol, (1.0, 1.0, 2.0), "AP", R._labels(dims, 6, 4)),
        geo=dict(sdd=1000.0, height=112, width=96, delx=2.2), patch_size=44, p_subsample=0.1, n_points=150,
        rot=rot, xyz=xyz)


@pytest.mark.parametrize("case", R.ROUTE_CASES, ids=R.route_case_id)
def test_gradient_route_on_the_device(gpu, scene, case):
    # (pose gradients: Siddon's on a volume with 1 % noise, from fp32 rays, differs from the float64
    # module's by the voxels its shortest segments pick -- 2e-3 ... 5.2e-3 here in the host build of the
    # same kernel cores -- so the allowance at this size is 1e-2)
    R.check_route_case(scene, case, gpu, ops, pose_tol=1e-2)


@pytest.mark.parametrize("name,dtype,grid", R.LAYOUT_IDS)
def test_renderer_layout_invariance_on_the_device(gpu, name, dtype, grid):
    exact_volume = name == "siddon_sum" and dtype == "f32" and grid
    R.check_renderer_layout(name, dtype, grid, gpu, exact=False, exact_volume=exact_volume, B=2)


@pytest.mark.parametrize("name", sorted(R.NCC_CASES))
def test_ncc_layout_invariance_on_the_device(gpu, name):
    R.check_ncc_layout(name, gpu, exact=False)


@pytest.mark.parametrize("lever", R.DRR_LAYOUT_LEVERS)
@pytest.mark.parametrize("renderer", ["siddon", "trilinear"])
def test_drr_pose_slices_layout_invariance_on_the_device(gpu, scene, renderer, lever):
    # (the Siddon volume gradient on the bricks: the fused route, and the general route's detector grid;
    # the pose gradient is a cancelling sum of every ray's float-atomic record: the strided and the
    # contiguous call, same values, have differed by 1.25e-5 of its largest component)
    R.check_drr_pose_layout(scene, renderer, lever, gpu, exact=False, n_poses=2, pose_tol=5e-5,
                            exact_volume=lambda fused: renderer == "siddon" and (fused or lever == "dense"))


def test_drr_ncc_fixed_slice_layout_invariance_on_the_device(gpu, scene):
    R.check_drr_ncc_layout(scene, gpu, exact=False)
