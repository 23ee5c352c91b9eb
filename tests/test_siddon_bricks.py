"""The Siddon brick entries per pixel against float64, on the host emulation (tests/emu: the same csrc headers compiled
for the CPU, 32^3 bricks for every storage), and the CPU-only tests of the reference itself: the float64 walk pinned to
the oracle, the float32 yardsticks, TIE and the left-out shares re-measured from the references alone.
tests/test_gpu_siddon_bricks.py runs the same checks of tests/siddon_brick_cases.py on the device."""
import numpy as np
import pytest

import siddon_brick_cases as sb

CASE_STORAGE = [(n, s) for n in sb.CASES for s in (sb.STORAGES_HOST if n in sb.GENERIC else ("f32", "q16"))]


def test_walk_is_the_oracle():
    """out, g_img, g_source and g_target of the float64 walk against oracle.siddon in float64 (the source expanded per
    ray): 1e-12 of each pixel's scale, on every scene, the dropped ones included."""
    for name in list(sb.GENERIC) + list(sb.CONSTRUCTED):
        ref = sb.reference(name)
        o = sb.oracle_rays(ref.sc, np.float64, ref.go)
        for q, got in o.items():
            S = np.broadcast_to(ref.S[q], got.shape)
            err = np.abs(got - ref.o64[q])
            worst = float((err[S > 0] / S[S > 0]).max())
            print(f"[{name}] {q}: walk against oracle {worst:.2e} of the scale")
            assert (err <= 1e-12 * S).all(), (name, q, worst)


def test_rho32_tie_and_left_out_shares():
    """The float32 yardstick of every quantity over every case, TIE, and the share of rays each generic scene's
    per-axis gates leave out: measured here from the references alone, held to what siddon_brick_cases writes down."""
    measured = {q: max(sb.reference(n).rho32[q] for n in sb.CASES) for q in sb.QUANTITIES}
    for q in sb.QUANTITIES:
        print(f"rho32 {q}: {measured[q]:.3e} = {measured[q] * 2 ** 24:.2f} x 2^-24 "
              f"(written: {sb.RHO32_MEASURED[q]:.3e}, cap {sb.RHO32_CAP[q]:.3e})")
        assert measured[q] <= sb.RHO32_CAP[q]
        assert measured[q] >= sb.RHO32_MEASURED[q] / 4  # (nor has the yardstick lost its teeth)
    # TIE: under the cap on the kept rays of every generic scene, at the plateau too, and half of it is not enough
    half = {q: 0.0 for q in ("g_source", "g_target")}
    for name in sb.GENERIC_CASES:
        ref = sb.reference(name)
        for q in half:
            at_tie, plateau = ref.rho32[q], sb.rho_of(ref, q, ref.tied_plateau)
            half[q] = max(half[q], sb.rho_of(ref, q, sb.tied(ref.w, sb.TIE / 2)))
            print(f"[{name}] rho32 {q}: {at_tie:.3e} with TIE, {plateau:.3e} with TIE_PLATEAU")
            assert at_tie <= sb.RHO32_CAP[q] and plateau <= sb.RHO32_CAP[q]
    print(f"with TIE / 2: {half}")
    assert any(half[q] > sb.RHO32_CAP[q] for q in half), "TIE is not the smallest power of two that holds"
    for name in sb.GENERIC_CASES:
        ref = sb.reference(name)
        share = sb.check_left_out(ref)  # (asserts the 2 % cap)
        lit = (ref.S["forward"] > 0).reshape(ref.sc.B, -1).mean(1)
        written = sb.LEFT_OUT_MEASURED[name]
        print(f"[{name}] left out {share:.4%} (written: {written:.4%}), pixels through the volume per pose "
              f"{np.round(lit, 2)}")
        assert abs(share - written) <= 0.02 * written + 1e-6
        assert lit.max() > 0.2, name
    lit = (sb.reference("generic_21x19").S["forward"] > 0).mean(1)
    assert lit[2] < 0.5 and lit[0] == 1.0  # the pose beside the volume: more than half its rays miss
    d = np.abs(sb.reference("generic_21x19").w.d[:, 199])
    assert d[3].argmax() == 2 and d[0].argmax() == 1  # pose 3 looks along z
    sc = sb.scene("generic_21x19")  # pose 4: the source inside the volume
    assert ((sc.source[4, 0] > -0.5) & (sc.source[4, 0] < np.asarray(sc.dims) - 0.5)).all()
    # the dropped scenes: the float32 and the float64 oracle disagree on the image itself beyond the cap
    for name in sb.DROPPED:
        ref = sb.reference(name)
        print(f"[{name}] dropped: rho32 forward {ref.rho32['forward']:.3e}")
        assert ref.rho32["forward"] > sb.RHO32_CAP["forward"]
    for name in sb.CONSTRUCTED:  # every number exact in float32, N < 16
        sc = sb.scene(name)
        assert sc.N == 9 and (sc.target * 4 == np.rint(sc.target * 4)).all()


@pytest.mark.parametrize("name,storage", CASE_STORAGE, ids=lambda v: v)
def test_forward_and_record_per_pixel(name, storage, emulated_ops):
    sb.check_forward_and_record(name, storage, "cpu", emulated_ops)


@pytest.mark.parametrize("storage", ("f32", "q16p"))
@pytest.mark.parametrize("name", sb.PACKED_CASES)
def test_packed_record_per_ray(name, storage, emulated_ops):
    sb.check_packed_record(name, storage, "cpu", emulated_ops)


@pytest.mark.parametrize("kind", sb.MASKS)
@pytest.mark.parametrize("name,storage", [("generic_21x19", "f32"), ("generic_24x20", "q16p"), ("sparse", "q16")],
                         ids=lambda v: v)
def test_masked_entry_per_pixel(name, storage, kind, emulated_ops):
    sb.check_masked(name, kind, storage, "cpu", emulated_ops)


@pytest.mark.parametrize("name", ["generic_21x19", "poses33_8x6"])
def test_record_into_buffers_cleared_by_the_ray_generation(name, emulated_ops):
    sb.check_cleared(name, "cpu", emulated_ops)


@pytest.mark.parametrize("name", sb.CHANNEL_CASES)
def test_channels_per_pixel(name, emulated_ops):
    sb.check_channels(name, "cpu", emulated_ops)
