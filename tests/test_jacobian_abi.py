"""The C ABI of the Jacobian determinant library: include/diffdrr_jacobian_hip.h <-> ctypes signatures <->
libdiffdrr_jacobian_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_jacobian_hip.h")
ENTRIES = {"ddrr_jacobian_abi_version", "ddrr_jacobian_last_error", "ddrr_jacobian_workspace_bytes",
           "ddrr_jacobian_determinant", "ddrr_jacobian_penalty", "ddrr_jacobian_backward"}
# (the forward kernel once per basis)
KERNELS = {"jacobian_forward_kernel": 2, "jacobian_fold_kernel": 1, "jacobian_rows_kernel": 1,
           "jacobian_gather_kernel": 1, "jacobian_pieces_kernel": 1, "jacobian_nodes_kernel": 1}


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def jacobian():
    import __graft_entry__ as entry

    entry.build_jacobian_hip()
    return _lib.jacobian_library(_lib.JACOBIAN_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.JACOBIAN_EXPORTS) == ENTRIES
    for name, argtypes in _lib._JACOBIAN_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    # ... and none of it is part of the other libraries' ABIs
    for other in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS, _lib.FBP_EXPORTS, _lib.LM_EXPORTS,
                  _lib.WARP_EXPORTS, _lib.BSPLINE_EXPORTS, _lib.POLYRIGID_EXPORTS):
        assert not set(decls) & set(other)
    P, I, L, D = _lib._P, _lib._I, _lib._L, _lib._D
    assert _lib._JACOBIAN_SIGNATURES["ddrr_jacobian_workspace_bytes"] == [I] * 7
    assert _lib._JACOBIAN_SIGNATURES["ddrr_jacobian_determinant"] == [P, I, I, I, I, I, I, I, P, P, L, P, P, P]
    assert _lib._JACOBIAN_SIGNATURES["ddrr_jacobian_penalty"] == [P, I, I, I, I, I, I, I, D, P, L, P, P, P, P]
    assert _lib._JACOBIAN_SIGNATURES["ddrr_jacobian_backward"] == [P, I, I, I, I, I, I, I, P, D, P, L, P, P]
    assert _lib._JACOBIAN_RESTYPES == {"ddrr_jacobian_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_JACOBIAN_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_JACOBIAN_ABI_VERSION"]) == _lib.JACOBIAN_ABI_VERSION == 1
    assert (int(const["DDRR_JACOBIAN_BASIS_LINEAR"]), int(const["DDRR_JACOBIAN_BASIS_BSPLINE"])) == \
        (_lib.JACOBIAN_BASIS_LINEAR, _lib.JACOBIAN_BASIS_BSPLINE) == (0, 1)
    assert int(const["DDRR_JACOBIAN_MAX_DIM"]) == _lib.JACOBIAN_MAX_DIM == 2**16 - 1
    assert int(const["DDRR_JACOBIAN_PARTIAL_BYTES"]) == _lib.JACOBIAN_PARTIAL_BYTES == 24
    # the domain is the warp entries'
    assert _lib.JACOBIAN_MAX_DIM == _lib.WARP_MAX_DIM == _lib.BSPLINE_MAX_DIM


def test_the_other_headers_and_their_versions_are_untouched():
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION,
            _lib.LM_ABI_VERSION, _lib.WARP_ABI_VERSION, _lib.BSPLINE_ABI_VERSION, _lib.POLYRIGID_ABI_VERSION) == \
        (33, 1, 1, 1, 1, 1, 1, 1)
    for other in (_lib.EXPORTS, _lib.WARP_EXPORTS, _lib.BSPLINE_EXPORTS, _lib.POLYRIGID_EXPORTS):
        assert not any(n.startswith("ddrr_jacobian") for n in other)
    assert set(_lib.BSPLINE_EXPORTS) == {"ddrr_bspline_abi_version", "ddrr_bspline_last_error",
                                         "ddrr_bspline_workspace_bytes", "ddrr_bspline_forward",
                                         "ddrr_bspline_backward_displacement", "ddrr_bspline_backward_volume"}
    assert set(_lib.WARP_EXPORTS) == {"ddrr_warp_abi_version", "ddrr_warp_last_error", "ddrr_warp_workspace_bytes",
                                      "ddrr_warp_forward", "ddrr_warp_backward_displacement",
                                      "ddrr_warp_backward_volume"}


def test_library_builds_loads_and_exports_exactly_the_header(jacobian):
    assert jacobian.cdll.ddrr_jacobian_abi_version() == _lib.JACOBIAN_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.JACOBIAN_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build():
    import inspect

    import __graft_entry__ as entry

    assert "build_jacobian_hip()" in inspect.getsource(entry.build)
    assert entry.JACOBIAN_LIB == _lib.JACOBIAN_LIB_PATH
    assert "jacobian_core.h" not in entry.HIP_HEADERS  # (the main library does not rebuild for it)
    assert "jacobian_library(JACOBIAN_LIB)" in inspect.getsource(entry.build)


def test_library_contains_gfx950_code_object(jacobian):
    blob = open(_lib.JACOBIAN_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)


def test_kernels_use_no_scratch_memory(jacobian):
    """Read the kernel descriptors of the built code object (as tests/test_bspline_abi.py does): no private
    segment in any kernel, and at most 128 registers (four waves per SIMD); the counts are printed."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.JACOBIAN_LIB_PATH, "rb").read()
    kernels = {}
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data):
        off = m.start()
        n = struct.unpack_from("<Q", data, off + 24)[0]
        p = off + 32
        for _ in range(n):
            o, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl].decode()
            p += tl
            if "gfx950" not in triple:
                continue
            path = os.path.join(ROOT, "tests", "emu", "_co_jacobian.elf")
            with open(path, "wb") as f:
                f.write(data[off + o:off + o + size])
            try:
                notes = subprocess.run([readelf, "--notes", path], capture_output=True, text=True).stdout
            finally:
                os.remove(path)
            name = None
            for line in notes.splitlines():  # kernel-level keys come in alphabetical order
                m2 = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_count):\s+(\S+)", line)
                if not m2:
                    continue
                key, val = m2.groups()
                if key == "name" and val.startswith("_Z"):
                    name = val
                elif key == "private_segment_fixed_size" and name is not None:
                    kernels[name] = [int(val), None]
                elif key == "vgpr_count" and name in kernels:
                    kernels[name][1] = int(val)
                    name = None
    for k, count in KERNELS.items():
        assert sum(k in name for name in kernels) == count, (k, sorted(kernels))
    assert len(kernels) == sum(KERNELS.values()), sorted(kernels)
    for name, (scratch, vgpr) in kernels.items():
        print(f"{name}: private_segment_fixed_size {scratch}, vgpr_count {vgpr}")
        assert scratch == 0, (name, scratch)
        assert vgpr is not None and vgpr <= 128, (name, vgpr)


def _args(name, a, null=None, D=(23, 30, 37), G=(4, 5, 3), basis=1, eps=0.1, ws_bytes=1 << 20, ws_off=8192):
    """Valid host-side arguments of a status entry (nothing is launched for the cases that use them)."""
    ptr = {"displacement": a, "det": a + 64, "gD": a + 128, "ws": a + ws_off, "gU": a + 256, "penalty": a + 320,
           "folded": a + 384, "range": a + 448}
    if null is not None:
        ptr[null] = None
    if name == "ddrr_jacobian_determinant":
        return (ptr["displacement"], *G, *D, basis, ptr["det"], ptr["ws"], ws_bytes, ptr["folded"], ptr["range"], None)
    if name == "ddrr_jacobian_penalty":
        return (ptr["displacement"], *G, *D, basis, eps, ptr["ws"], ws_bytes, ptr["penalty"], ptr["folded"],
                ptr["range"], None)
    return (ptr["displacement"], *G, *D, basis, ptr["gD"], eps, ptr["ws"], ws_bytes, ptr["gU"], None)


# (gD may be NULL: it selects the penalty's gradient)
POINTERS = {"ddrr_jacobian_determinant": ("displacement", "det", "ws", "folded", "range"),
            "ddrr_jacobian_penalty": ("displacement", "ws", "penalty", "folded", "range"),
            "ddrr_jacobian_backward": ("displacement", "ws", "gU")}


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(jacobian):
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._JACOBIAN_SIGNATURES if n not in _lib._JACOBIAN_RESTYPES]
    assert status_entries == list(POINTERS)
    for name in status_entries:
        argtypes = _lib._JACOBIAN_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (0.1 if t is _lib._D else ints) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(jacobian.cdll, name)(*args)
            msg = jacobian.cdll.ddrr_jacobian_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            jacobian.call(name, *[None if t is _lib._P else (0.1 if t is _lib._D else 0) for t in argtypes])
    assert jacobian.query("ddrr_jacobian_workspace_bytes", -1, 30, 37, 4, 5, 3, 1) == -1
    # B-spline, 23 x 30 x 37 with (4, 5, 3): r1 (3, 3, Dx, Dy, Gz) | r2 (2, 3, Dx, Gy, Gz) floats
    #   = 4 * 3 * 23 * 3 * (3 * 30 + 2 * 5); the forward partials, 24 * 1 * 8 * 23, are fewer
    assert jacobian.query("ddrr_jacobian_workspace_bytes", 23, 30, 37, 4, 5, 3, 1) == 4 * 3 * 23 * 3 * 100 == 82800
    # linear, same shape: 24 cells of at most 8 x 8 x 19 voxels -> 2 pieces of 24 floats each = 4608 bytes: the
    # 184 partials of 24 bytes, 4416, are fewer
    assert jacobian.query("ddrr_jacobian_workspace_bytes", 23, 30, 37, 4, 5, 3, 0) == 4 * 24 * 24 * 2 == 4608
    # 2 x 2 x 2: one partial (24 bytes) against r1 | r2 = 4 * 3 * 2 * 2 * (6 + 4) = 480, or one piece (96)
    assert jacobian.query("ddrr_jacobian_workspace_bytes", 2, 2, 2, 2, 2, 2, 1) == 480
    assert jacobian.query("ddrr_jacobian_workspace_bytes", 2, 2, 2, 2, 2, 2, 0) == 96
    # a long thin volume with a coarse lattice: the forward partials are the larger part
    assert jacobian.query("ddrr_jacobian_workspace_bytes", 65535, 2, 3, 2, 2, 2, 0) == 24 * 65535


def test_argument_rules(jacobian):
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    cases = [(name, _args(name, a, null=n), "null pointer") for name, ptrs in POINTERS.items() for n in ptrs]
    for name in POINTERS:
        cases += [
            (name, _args(name, a, D=(23, -30, 37)), "positive"),
            (name, _args(name, a, G=(4, 5, -3)), "positive"),
            (name, _args(name, a, G=(4, 1, 3)), "G_a >= 2"),
            (name, _args(name, a, G=(4, 5, 0)), "G_a >= 2"),
            (name, _args(name, a, G=(24, 5, 3)), "G_a <= D_a"),
            (name, _args(name, a, G=(4, 5, 38)), "G_a <= D_a"),
            (name, _args(name, a, D=(2, 2, 65536), G=(2, 2, 2)), "2\\^16"),
            (name, _args(name, a, D=(65536, 30, 37)), "2\\^16"),
            (name, _args(name, a, D=(2048, 2048, 513)), "2\\^31 voxels"),
            (name, _args(name, a, basis=2), "basis"),
            (name, _args(name, a, basis=-1), "basis"),
            (name, _args(name, a, ws_bytes=82800 - 1), "ws_bytes"),
            (name, _args(name, a, ws_bytes=-1), "ws_bytes"),
            (name, _args(name, a, ws_off=8196), "8-byte aligned"),
        ]
    for name in ("ddrr_jacobian_penalty", "ddrr_jacobian_backward"):
        cases += [(name, _args(name, a, eps=e), r"eps must be in \(0, 1\]")
                  for e in (0.0, -0.1, 1.0000001, float("nan"), float("inf"))]
    for name, args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            jacobian.call(name, *args)
    # exactly 2^31 voxels is inside the domain (the query launches nothing)
    assert jacobian.query("ddrr_jacobian_workspace_bytes", 1024, 1024, 2048, 2, 2, 2, 1) == \
        4 * 3 * 1024 * 2 * (3 * 1024 + 2 * 2)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_jacobian_lib", None)
    monkeypatch.setattr(_lib, "JACOBIAN_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_jacobian_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops._query_jacobian("ddrr_jacobian_workspace_bytes", 2, 2, 2, 2, 2, 2, 0)
