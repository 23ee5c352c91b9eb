"""Levenberg-Marquardt registration on the MI355X: the checks of tests/test_lm.py through the gfx950 kernels
(libdiffdrr_lm_hip.so), and the device's partial sums against the same order on the host."""
import pytest
import torch

import lm_cases
from diffdrr_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(lm_cases.SUM_CASES))
def test_sums_and_jacobian_against_float64(gpu, name):
    lm_cases.check_sums_and_jacobian(name, gpu, ops)


def test_step_sequences_against_the_definition(gpu):
    lm_cases.check_step_sequences(gpu, ops)


def test_convergence_in_half_of_adams_iterations(gpu):
    lm_cases.check_convergence(gpu)


def test_device_sums_equal_the_host_build_bit_for_bit_given_the_same_rows(gpu):
    """The staged Gram sums are exact products added in a fixed order: from the device's own per-ray rows
    (j, x, f) the partials must be exactly what the same order gives in float64 on the host."""
    name = "4087_rays_four_workgroups"
    drr_cpu, rot, xyz, conv = lm_cases.sum_scene(name)
    import copy
    drr = copy.deepcopy(drr_cpu).to(gpu)
    rot, xyz = rot.to(gpu), xyz.to(gpu)
    aux, args, kw, x32 = lm_cases.render_record(drr, rot, xyz, conv, ops)
    B, N = x32.shape
    fixed = torch.rand(B, N, generator=torch.Generator().manual_seed(4)).to(gpu)
    ws, jac = ops.lm_normal_sums(aux, fixed, **args, **kw, want_jacobian=True)
    u = torch.cat([jac.double(), x32.double()[..., None], fixed.double()[..., None],
                   torch.ones(B, N, 1, dtype=torch.float64, device=gpu)], -1).cpu()
    pq = torch.tensor(lm_cases.pair_table())
    G = ws.shape[1]
    want = torch.zeros(B, G, 44, dtype=torch.float64)
    for b in range(B):
        for w in range(G):
            rows = u[b, w * 1024:(w + 1) * 1024]
            prod = rows[:, pq[:, 0]] * rows[:, pq[:, 1]]  # (count, 44), exact in double
            slices = []
            for s in range(5):
                acc = torch.zeros(44, dtype=torch.float64)
                for row in prod[s::5]:
                    acc = acc + row
                slices.append(acc)
            total = slices[0]
            for s in range(1, 5):
                total = total + slices[s]
            want[b, w] = total
    assert torch.equal(ws.cpu(), want)
