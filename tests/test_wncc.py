"""The weighted (masked) NCC without a GPU: the host build of csrc/wncc_core.h (tests/emu/wncc_emu.cpp) behind the
product's own Python layers -- the fused entries against the chain in float64 under every weight pattern, masked
pixels that are never read, scale and repeat, the image entries on DRR-like images, the module route and its
fallbacks, a registration that needs the mask.  The checks are tests/wncc_cases.py's, shared with the device."""
import pytest
import torch

import diffdrr_amd
import wncc_cases
from diffdrr_amd import _lib

CPU = torch.device("cpu")


@pytest.fixture()
def wncc_ops(emulated_ops, monkeypatch):
    wncc_cases.route_wncc_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_exported_from_the_package():
    ops = diffdrr_amd.ops
    assert _lib.WNCC_ABI_VERSION == 1 and _lib.WNCC_GROUP_RAYS == 1024 and _lib.WNCC_STATS == 6
    assert all(callable(getattr(ops, n)) for n in ("wncc_workspace", "wncc_forward", "wncc_backward",
                                                   "siddon_wncc_forward", "siddon_wncc_backward_pose"))
    assert callable(diffdrr_amd.metrics.weighted_ncc)


def test_weight_patterns_are_what_they_are_called():
    B, H, W = 3, 30, 26
    w = {p: wncc_cases.weights(p, B, H, W, True, CPU) for p in wncc_cases.PATTERNS}
    assert all(t.shape == (B, H * W) and t.dtype == torch.float32 and bool((t >= 0).all()) for t in w.values())
    assert bool((w["ones"] == 1).all()) and 0.55 < float(w["disc"].mean()) < 0.7 and set(w["disc"].unique().tolist()) == {0, 1}
    assert float(w["smooth"].min()) >= 0.25 and float(w["smooth"].max()) <= 1.75
    assert 0.4 < float(w["half"].mean()) < 0.6
    hot = w["edge-hot"] != 0
    assert hot[0].nonzero().flatten().tolist() == wncc_cases.F.edge_set(H * W)
    assert float(w["edge-hot"][hot].min()) >= 0.5 and float(w["edge-hot"][hot].max()) <= 1.5
    assert bool((w["one pose empty"][-1] == 0).all()) and bool((w["one pose empty"][:-1].sum(1) > 0).all())
    assert wncc_cases.weights("one pose empty", 1, H, W, True, CPU) is None
    assert wncc_cases.weights("one pose empty", B, H, W, False, CPU) is None
    assert bool((wncc_cases.weights("disc", 1, 2, 3, False, CPU) == 1).all())
    # ... and the composition reads them as the definition does: ones is the plain NCC, a scaled weight changes nothing
    x = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    plain = diffdrr_amd.metrics.NormalizedCrossCorrelation2d()(x, y)
    assert torch.allclose(diffdrr_amd.metrics.weighted_ncc(x, y, w["ones"].double().reshape(B, 1, H, W)), plain, atol=1e-12)
    smooth = w["smooth"].double().reshape(B, 1, H, W)
    assert torch.allclose(diffdrr_amd.metrics.weighted_ncc(x, y, 4 * smooth), diffdrr_amd.metrics.weighted_ncc(x, y, smooth),
                          atol=1e-14)


@pytest.mark.parametrize("name", wncc_cases.HOST_CASES)
def test_weights_are_a_sharp_check_in_float64(wncc_ops, name):
    wncc_cases.check_sharpness(name, CPU, wncc_ops)


@pytest.mark.parametrize("name", wncc_cases.HOST_CASES)
def test_fused_forward_against_float64(wncc_ops, name):
    wncc_cases.check_forward(name, CPU, wncc_ops)


@pytest.mark.parametrize("name", wncc_cases.HOST_CASES)
def test_fused_backward_against_float64(wncc_ops, name):
    wncc_cases.check_backward(name, CPU, wncc_ops)


@pytest.mark.parametrize("name", wncc_cases.HOST_CASES)
def test_masked_pixels_are_not_read(wncc_ops, name):
    wncc_cases.check_masked_pixels_are_not_read(name, CPU, wncc_ops)


@pytest.mark.parametrize("name", wncc_cases.HOST_CASES)
def test_scaled_weights_and_repeated_calls_give_the_same_bits(wncc_ops, name):
    wncc_cases.check_scale_and_repeat(name, CPU, wncc_ops)


@pytest.mark.parametrize("shape,setting", wncc_cases.IMAGE_CASES,
                         ids=[f"{'x'.join(map(str, s))}-{t}" for s, t in wncc_cases.IMAGE_CASES])
def test_image_entries_against_float64(wncc_ops, shape, setting):
    wncc_cases.check_image_entries(shape, setting, CPU, wncc_ops)


def test_torch_composition_is_the_float64_definition():
    wncc_cases.check_composition_is_the_definition(CPU)


def test_criteria_with_a_weight_and_their_routes(wncc_ops):
    wncc_cases.check_criteria_and_routes(CPU, wncc_ops)


def test_module_route_and_fallbacks(wncc_ops):
    wncc_cases.check_module_route(CPU, wncc_ops)


def test_registration_with_a_mask_converges_and_does_not_read_the_bar(wncc_ops):
    wncc_cases.check_registration(CPU, wncc_ops)


def test_the_registration_scene_needs_the_mask(wncc_ops):
    wncc_cases.check_scene_needs_the_mask(CPU, wncc_ops)


def test_ops_refuse_other_records_and_shapes_without_a_launch(wncc_ops):
    wncc_cases.check_layout_errors(wncc_ops)


def test_workspace_is_cached_per_shape_and_sized_by_the_library(wncc_ops):
    ws = wncc_ops.wncc_workspace(3, 1025, "cpu")
    assert ws.dtype == torch.float64 and ws.numel() * 8 == 3 * 2 * _lib.WNCC_SLOT_BYTES
    assert wncc_ops.wncc_workspace(3, 1025, "cpu") is ws and wncc_ops.wncc_workspace(3, 1024, "cpu") is not ws
    assert wncc_ops.wncc_workspace(0, 10, "cpu").numel() == 0
    ncc, stats = wncc_ops.wncc_forward(torch.ones(1, 8), torch.ones(0, 8), torch.ones(1, 8), 1e-5)
    assert ncc.shape == (0,) and stats.shape == (0, 6)
