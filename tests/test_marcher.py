"""The marcher's brick entries and the per-ray entries they are compared with, per pixel against float64, on the
host emulation (tests/emu: the same csrc headers compiled for the CPU).  tests/test_gpu_marcher.py runs the same
checks of tests/marcher_cases.py on the device."""
import pytest

import marcher_cases as mc

ids = mc.case_id


def test_rho32_and_left_out_shares():
    """The float32 yardstick of every quantity over every case, and the share of rays each scene's gradient gates
    leave out: measured here from the oracle alone, held to the values written into marcher_cases."""
    measured = mc.rho32_all()
    for q in mc.QUANTITIES:
        print(f"rho32 {q}: {measured[q]:.3e} = {measured[q] * 2 ** 24:.2f} x 2^-24 (written: {mc.RHO32_MEASURED[q]:.3e}, "
              f"cap {mc.RHO32_CAP[q]:.3e})")
        assert measured[q] <= mc.RHO32_CAP[q]
        assert measured[q] >= mc.RHO32_MEASURED[q] / 4  # (nor has the yardstick lost its teeth)
    for case in mc.CASES:
        ref = mc.reference(case)
        share = mc.check_left_out(ref)
        lit = float((ref.S["forward"] > 0).mean())
        print(f"[{ref.sc.name}] left out {share:.2%} (written: {mc.LEFT_OUT_MEASURED.get(ref.sc.name, 0.0):.2%}), "
              f"pixels with a sample in the volume {lit:.0%}")
        assert lit > 0.2 or ref.sc.amin == ref.sc.amax, ref.sc.name  # every scene hits its volume (step = 0: S = 0)
        assert abs(share - mc.LEFT_OUT_MEASURED.get(ref.sc.name, 0.0)) < 5e-3


@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_forward_per_pixel(case, emulated_ops):
    mc.check_forward(case, "cpu", emulated_ops)


@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_ray_gradients_per_pixel(case, emulated_ops):
    mc.check_ray_gradients(case, "cpu", emulated_ops)


@pytest.mark.parametrize("case", mc.CHANNEL_CASES, ids=ids)
def test_channels_per_pixel(case, emulated_ops):
    mc.check_channels(case, "cpu", emulated_ops)


@pytest.mark.parametrize("case", mc.ORDERING_CASES, ids=ids)
def test_a_pose_alone_equals_the_pose_in_a_batch(case, emulated_ops):
    mc.check_ordering(case, "cpu", emulated_ops)


@pytest.mark.parametrize("case", mc.OWNER_BOX_CASES, ids=ids)
def test_owner_box_volume_gradient_per_voxel(case, emulated_ops):
    mc.check_owner_box(case, "cpu", emulated_ops)
