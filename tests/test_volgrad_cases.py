"""The float64 reference of the brick volume-gradient tests (tests/volgrad_cases.py) pinned to the oracle, and
the conditions its scenes are frozen under.  No GPU: tests/test_gpu_volume_gradient_bricks.py holds the
kernels against this reference on the device."""
import numpy as np
import pytest

import volgrad_cases as vc
from conftest import rel_err

PINNED = [k for k in vc.KINDS if k != "marcher_channels"]  # (the oracle has no marcher with channels)


@pytest.mark.parametrize("kind", PINNED)
@pytest.mark.parametrize("name", vc.SCENE_NAMES)
def test_walker_is_the_oracle(name, kind):
    """g64 is the oracle's g_volume on the same float64 inputs to 1e-10 of its maximum, and A -- with it the hit
    lists n and T are summed from -- is the oracle's g_volume for |grad_out|."""
    sc = vc.scene(name, kind)
    go, _ = vc.grad_out(sc, kind, "G3")
    w = vc.walk(sc, kind, go)
    ref = vc.oracle_volume_gradient(sc, kind, go)
    assert np.abs(ref).max() > 0
    assert rel_err(w.g64, ref) < 1e-10
    assert rel_err(w.A, vc.oracle_volume_gradient(sc, kind, np.abs(go))) < 1e-10
    assert ((w.n > 0) == (w.A > 0)).all() and ((w.T > 0) == (w.A > 0)).all()


@pytest.mark.parametrize("name", ["far3", "thick"])
def test_marcher_channels_with_one_label_is_the_plain_marcher(name, monkeypatch):
    """The one entry without an oracle: with every voxel labelled k (k = 0 is also the label outside the volume) the
    channel walk is the plain walk of grad_out's row k, and a label without a channel gives nothing."""
    sc = vc.scene(name)
    go, _ = vc.grad_out(sc, "marcher_channels", "G1")
    for k in (0, 3, vc.N_CHANNELS):
        monkeypatch.setattr(sc, "labels", np.full(sc.dims, k, np.uint8))
        vc._hit_cache.clear()
        w = vc.walk(sc, "marcher_channels", go)
        vc._hit_cache.clear()
        # (samples whose nearest voxel lies outside the volume take row 0 whatever the map says)
        inside = np.zeros(sc.dims, bool)
        inside[1:-1, 1:-1, 1:-1] = True
        if k == vc.N_CHANNELS:
            assert not w.g64[inside].any() and not w.n[inside].any()
            continue
        inner = vc.walk(sc, "marcher", go[:, k])
        assert inner.g64[inside].any()
        if k == 0:
            assert np.array_equal(w.g64, inner.g64)
        else:
            assert np.array_equal(w.g64[inside], inner.g64[inside])
    vc._hit_cache.clear()


@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("name", vc.SCENE_NAMES)
def test_every_scene_hits_the_volume(name, kind):
    sc = vc.scene(name, kind)
    go, _ = vc.grad_out(sc, kind, "G2")
    w = vc.walk(sc, kind, go)
    assert (w.n > 0).sum() > 200, name
    assert (w.A[w.n > 0] > 0).all()
    bricks = tuple(-(-d // 32) for d in sc.dims)
    assert bricks == ((2, 3, 2) if sc.dims[0] == 40 else (1, 1, 1)) and all(d % 32 for d in sc.dims)


@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("pattern", ["G3", "G3p", "G4"])
def test_faint_patterns_leave_voxels_that_only_faint_rays_cross(pattern, kind):
    sc = vc.scene("far3")
    go, bright = vc.grad_out(sc, kind, pattern)
    w = vc.walk(sc, kind, go, bright)
    assert ((w.n > 0) & (w.nb == 0)).sum() >= 200
    assert (w.nb > 0).sum() >= 20  # ... and some that bright rays cross


def test_near_and_near_float_straddle_one_voxel_of_distance():
    near, near_float = vc.scene("near"), vc.scene("near_float")
    assert 1.0 < vc.source_gap(near) <= 2.0 and 0.0 < vc.source_gap(near_float) <= 1.0
    assert abs(vc.source_gap(near) - vc.source_gap(near_float) - 1.0) < 1e-2  # one whole voxel closer
    for renderer in ("siddon", "marcher"):  # ... and nothing else sends `near` to the float path
        assert vc.rays_through_a_voxel(near, renderer) < 16384 * 0.9
    assert vc.source_gap(vc.scene("inside")) == 0.0


@pytest.mark.parametrize("renderer", ["siddon", "marcher"])
def test_switch_straddles_the_pose_bound(renderer):
    """B_lo poses of `switch` sum to n_sum <= 16384, one more to n_sum > 16384, with at least three pose chunks of
    32, and ceil(R) is not a rounding error away from another whole number."""
    R = vc.rays_through_a_voxel(vc.scene("switch_lo", renderer), renderer)
    assert int(np.ceil(R)) == vc.SWITCH_R[renderer] and 1e-3 < np.ceil(R) - R < 1 - 1e-3
    b_lo, b_hi = vc.switch_poses(renderer, "switch_lo"), vc.switch_poses(renderer, "switch_hi")
    assert b_lo > 64 and b_hi == b_lo + 1
    assert b_lo * vc.SWITCH_R[renderer] <= 16384 < b_hi * vc.SWITCH_R[renderer]
    assert vc.scene("switch_hi", renderer).B == b_hi


def test_fixed_scenes_have_a_bound_and_float_scenes_do_not():
    for name in vc.SCENES:
        sc = vc.scene(name)
        for renderer in ("siddon", "marcher"):
            n_sum = sum(np.ceil(vc.rays_through_a_voxel(sc, renderer, u)) for u in range(sc.B))
            assert (n_sum <= 16384) == sc.fixed, (name, renderer, n_sum)
