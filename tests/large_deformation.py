"""One volume past 2^30 voxels for each deformation library (tests/test_gpu_warp.py, test_gpu_bspline.py,
test_gpu_polyrigid.py): byte offsets beyond 2 GiB and 4 GiB in the forward kernels, the lattice gradients and
the atomic scatter.

The volume is (1040, 1024, 1024), random on the device; the upstream gradient gW is zero except in four
windows -- the first corner, around the voxels of linear index 2^29 (512, 0, 0) and 2^30 (1024, 0, 0), and the
last corner with the very last voxel.  W is compared on the windows, gV on the windows grown by the largest
displacement + 2 (and nowhere else may gV be other than 0), the lattice gradients as a whole, each against the
library's definition evaluated on those windows only (``box=``) from the part of the volume they reach
(``part=``), in float64 and in float32 from the same float32 tensors, under the project's gate
(warp_cases.gate).  No dense float64 copy of the volume exists; the peak is four volumes and the workspaces."""
import math

import pytest
import torch

from warp_cases import gate

SHAPE = (1040, 1024, 1024)
GRID = (5, 4, 6)
SIDE = 20
WINDOWS = {
    "first corner": tuple((0, SIDE) for _ in SHAPE),
    "index 2^29": ((512 - SIDE // 2, 512 + SIDE // 2), (0, SIDE), (0, SIDE)),
    "index 2^30": ((1024 - SIDE // 2, 1024 + SIDE // 2), (0, SIDE), (0, SIDE)),
    "last corner": tuple((D - SIDE, D) for D in SHAPE),
}
# the closest a sample coordinate of a window may come to a voxel face, where the lattice gradients jump: four
# float32 ulps of a displacement of 4 to 8 voxels (within that, a float32 evaluation of the field may fall on
# either side).  The scenes' seeds are the first ones from 1 that keep it (checked without the volume).
FACE_MARGIN = 4 * 2.0 ** -21
assert (512 * SHAPE[1] + 0) * SHAPE[2] + 0 == 2 ** 29 and (1024 * SHAPE[1] + 0) * SHAPE[2] + 0 == 2 ** 30


def slices(box):
    return tuple(slice(a, b) for a, b in box)


def grown(box, by):
    return tuple((max(a - by, 0), min(b + by, D)) for (a, b), D in zip(box, SHAPE))


def displacements(field):
    """Per window of the float64 field ``field(box)``: (largest |u|, smallest distance of a sample coordinate to a
    voxel face).  x is an integer: x + u is as far from one as u."""
    return {name: (float(u.abs().max()), float((u - u.round()).abs().min()))
            for name, u in ((name, field(box)) for name, box in WINDOWS.items())}


def device_scene(device, seed):
    """(V, gW) on the device, or a skip where five volumes' worth of memory is not free."""
    voxels = SHAPE[0] * SHAPE[1] * SHAPE[2]
    free, _ = torch.cuda.mem_get_info(device)
    need = 5 * 4 * voxels + (2 << 30)  # V, W, gW, gV, one more for what the allocator keeps; the workspaces
    if free < need:
        pytest.skip(f"needs {need / 2**30:.0f} GiB of device memory, {free / 2**30:.0f} free")
    g = torch.Generator(device=device).manual_seed(seed)
    V = torch.rand(SHAPE, device=device, generator=g)
    gW = torch.zeros(SHAPE, device=device)
    for box in WINDOWS.values():
        gW[slices(box)] = torch.rand([b - a for a, b in box], device=device, generator=g)
    return V, gW


def lattice(seed, amplitude):
    """(3, *GRID) float32 on the CPU, seeded, uniform in +-amplitude voxels."""
    return (torch.rand(3, *GRID, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * amplitude


def default_lattice_gate(name, names, got, ref64, ref32, held):
    for what, a, b, c in zip(names, got, ref64, ref32):
        gate(name, what, a, b, float((c.double() - b).abs().max()))


def check(name, device, seed, params, names, kernel, definition, field, float32_definition=None,
          lattice_gate=default_lattice_gate):
    """``kernel(V, *params)`` -> W on the device (differentiable) against ``definition(part of V, *params,
    box=, part=)`` -> W on the box, in the dtype of ``params`` (``float32_definition`` for float32, where it is
    another evaluation of the same function).  ``params``: the float32 lattice parameters on the CPU, ``names``
    what their gradients are called; ``field(box)`` -> the float64 displacement field u on a box;
    ``lattice_gate(name, names, gradients, float64 sums, float32 sums, held)`` gates the lattice gradients, ``held``
    being the windows' (box, reach, part of V, gW) on the CPU."""
    seen = displacements(field)
    largest = max(m for m, _ in seen.values())
    print(f"{name}: largest displacement in the windows {largest:.2f} voxels, closest sample coordinate to a voxel "
          f"face {min(d for _, d in seen.values()):.1e} voxel")
    assert 1.0 < largest < 8.5 and min(d for _, d in seen.values()) >= FACE_MARGIN
    V, gW = device_scene(device, seed)
    V.requires_grad_()
    on_device = [p.to(device).requires_grad_() for p in params]
    W = kernel(V, *on_device)
    assert W.shape == V.shape and W.dtype == torch.float32
    gV, *g_params = torch.autograd.grad(W, (V, *on_device), gW)
    W = W.detach()
    V.requires_grad_(False)
    sums = {torch.float64: None, torch.float32: None}
    inside, held = 0, []
    for window, box in WINDOWS.items():
        reach = grown(box, math.ceil(seen[window][0]) + 2)
        part, upstream = V[slices(reach)].cpu(), gW[slices(box)].cpu()
        held.append((box, reach, part, upstream))
        results = {}
        for dtype in sums:
            leaves = [t.detach().to(dtype, copy=True).requires_grad_() for t in (part, *params)]
            evaluate = float32_definition if dtype == torch.float32 and float32_definition else definition
            Wd = evaluate(*leaves, box=box, part=(SHAPE, reach))
            assert Wd.dtype == dtype and Wd.shape == upstream.shape
            grads = torch.autograd.grad(Wd, leaves, upstream.to(dtype))
            results[dtype] = (Wd.detach().double(), grads[0].double())
            sums[dtype] = list(grads[1:]) if sums[dtype] is None else [a + b for a, b in zip(sums[dtype], grads[1:])]
        (W64, gV64), (W32, gV32) = results[torch.float64], results[torch.float32]
        gate(f"{name} {window}", "W", W[slices(box)], W64, float((W32 - W64).abs().max()))
        gate(f"{name} {window}", "gV", gV[slices(reach)], gV64, float((gV32 - gV64).abs().max()))
        inside += int(torch.count_nonzero(gV[slices(reach)]))
    everywhere = int(torch.count_nonzero(gV))
    print(f"{name}: gV is not zero at {everywhere} voxels, {inside} of them in the grown windows")
    assert everywhere == inside and inside > 0
    lattice_gate(name, names, g_params, sums[torch.float64], sums[torch.float32], held)


def check_domain_errors(monkeypatch, ops, launcher, forward, checker, lattice):
    """A 65536-long axis and (1025, 2048, 1024) = 2^31 + 2^21 voxels raise the named ValueError from ``ops``
    before anything is launched.  ``forward(V)`` calls the library's forward entry with a lattice on V's device;
    ``checker(shape)`` is its domain check on a shape alone (no 8 GiB tensor is made)."""
    def launched(*a):
        raise AssertionError("launched")

    monkeypatch.setattr(ops, launcher, launched)
    for shape in ((65536, 2, 2), (2, 65536, 2), (2, 2, 65536)):
        with pytest.raises(ValueError, match="at most 65535 voxels per axis"):
            forward(torch.zeros(shape, device=lattice.device))
    with pytest.raises(ValueError, match=r"at most 2\^31 voxels"):
        checker((1025, 2048, 1024))
    checker((1024, 2048, 1024))  # exactly 2^31 voxels is inside the domain
