"""The C ABI of the cubic B-spline deformation library: include/diffdrr_bspline_hip.h <-> ctypes signatures <->
libdiffdrr_bspline_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_bspline_hip.h")
ENTRIES = {"ddrr_bspline_abi_version", "ddrr_bspline_last_error", "ddrr_bspline_workspace_bytes",
           "ddrr_bspline_forward", "ddrr_bspline_backward_displacement", "ddrr_bspline_backward_volume"}
KERNELS = ("bspline_forward_kernel", "bspline_rows_kernel", "bspline_gather_kernel", "bspline_volume_kernel")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def bspline():
    import __graft_entry__ as entry

    entry.build_bspline_hip()
    return _lib.bspline_library(_lib.BSPLINE_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.BSPLINE_EXPORTS) == ENTRIES
    for name, argtypes in _lib._BSPLINE_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    # ... and none of it is part of the other six libraries' ABIs
    for other in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS, _lib.FBP_EXPORTS, _lib.LM_EXPORTS,
                  _lib.WARP_EXPORTS):
        assert not set(decls) & set(other)
    P, I, L = _lib._P, _lib._I, _lib._L
    assert _lib._BSPLINE_SIGNATURES["ddrr_bspline_workspace_bytes"] == [I] * 6
    assert _lib._BSPLINE_SIGNATURES["ddrr_bspline_forward"] == [P, I, I, I, P, I, I, I, I, P, P]
    assert _lib._BSPLINE_SIGNATURES["ddrr_bspline_backward_displacement"] == [P, I, I, I, P, I, I, I, I, P, P, L, P, P]
    assert _lib._BSPLINE_SIGNATURES["ddrr_bspline_backward_volume"] == [P, I, I, I, I, I, I, I, P, P, P]
    assert _lib._BSPLINE_RESTYPES == {"ddrr_bspline_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_BSPLINE_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_BSPLINE_ABI_VERSION"]) == _lib.BSPLINE_ABI_VERSION == 1
    assert (int(const["DDRR_BSPLINE_PADDING_ZEROS"]), int(const["DDRR_BSPLINE_PADDING_BORDER"])) == \
        (_lib.BSPLINE_PADDING_ZEROS, _lib.BSPLINE_PADDING_BORDER) == (0, 1)
    assert int(const["DDRR_BSPLINE_MAX_DIM"]) == _lib.BSPLINE_MAX_DIM == 2**16 - 1
    assert int(const["DDRR_BSPLINE_CHUNK_VOXELS"]) == _lib.BSPLINE_CHUNK_VOXELS == 256
    assert int(const["DDRR_BSPLINE_ROWS"]) == _lib.BSPLINE_ROWS == 4
    # the two bases share the padding codes and the domain
    assert (_lib.BSPLINE_PADDING_ZEROS, _lib.BSPLINE_PADDING_BORDER, _lib.BSPLINE_MAX_DIM) == \
        (_lib.WARP_PADDING_ZEROS, _lib.WARP_PADDING_BORDER, _lib.WARP_MAX_DIM)


def test_the_other_headers_and_their_versions_are_untouched():
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION,
            _lib.LM_ABI_VERSION, _lib.WARP_ABI_VERSION) == (33, 1, 1, 1, 1, 1)
    assert not any(n.startswith("ddrr_bspline") for n in _lib.EXPORTS)
    assert set(_lib.WARP_EXPORTS) == {"ddrr_warp_abi_version", "ddrr_warp_last_error", "ddrr_warp_workspace_bytes",
                                      "ddrr_warp_forward", "ddrr_warp_backward_displacement",
                                      "ddrr_warp_backward_volume"}
    counts = {"EXPORTS": len(_lib.EXPORTS), "MI": len(_lib.MI_EXPORTS), "RECON": len(_lib.RECON_EXPORTS),
              "FBP": len(_lib.FBP_EXPORTS), "LM": len(_lib.LM_EXPORTS)}
    assert all(counts.values()), counts


def test_library_builds_loads_and_exports_exactly_the_header(bspline):
    assert bspline.cdll.ddrr_bspline_abi_version() == _lib.BSPLINE_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.BSPLINE_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build():
    import inspect

    import __graft_entry__ as entry

    assert "build_bspline_hip()" in inspect.getsource(entry.build)
    assert entry.BSPLINE_LIB == _lib.BSPLINE_LIB_PATH
    assert "bspline_core.h" not in entry.HIP_HEADERS and "warp_core.h" not in entry.HIP_HEADERS
    # (the main library does not rebuild for either)


def test_library_contains_gfx950_code_object(bspline):
    blob = open(_lib.BSPLINE_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)


def test_kernels_use_no_scratch_memory(bspline):
    """Read the kernel descriptors of the built code object (as tests/test_lm_abi.py does): no private
    segment in any kernel, and at most 128 registers (four waves per SIMD); the counts are printed."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.BSPLINE_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_bspline.elf")
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
    for k in KERNELS:
        assert sum(k in name for name in kernels) == 1, (k, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name, (scratch, vgpr) in kernels.items():
        print(f"{name}: private_segment_fixed_size {scratch}, vgpr_count {vgpr}")
        assert scratch == 0, (name, scratch)
        assert vgpr is not None and vgpr <= 128, (name, vgpr)


def _args(name, a, null=None, D=(23, 30, 37), G=(4, 5, 3), padding=0, ws_bytes=1 << 20, ws_off=8192):
    """Valid host-side arguments of a status entry (nothing is launched for the cases that use them)."""
    ptr = {"V": a, "displacement": a + 64, "W": a + 128, "gW": a + 192, "ws": a + ws_off, "gU": a + 256, "gV": a + 320}
    if null is not None:
        ptr[null] = None
    if name == "ddrr_bspline_forward":
        return (ptr["V"], *D, ptr["displacement"], *G, padding, ptr["W"], None)
    if name == "ddrr_bspline_backward_displacement":
        return (ptr["V"], *D, ptr["displacement"], *G, padding, ptr["gW"], ptr["ws"], ws_bytes, ptr["gU"], None)
    return (ptr["displacement"], *G, *D, padding, ptr["gW"], ptr["gV"], None)


POINTERS = {"ddrr_bspline_forward": ("V", "displacement", "W"),
            "ddrr_bspline_backward_displacement": ("V", "displacement", "gW", "ws", "gU"),
            "ddrr_bspline_backward_volume": ("displacement", "gW", "gV")}


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(bspline):
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._BSPLINE_SIGNATURES if n not in _lib._BSPLINE_RESTYPES]
    assert status_entries == list(POINTERS)
    for name in status_entries:
        argtypes = _lib._BSPLINE_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else ints for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(bspline.cdll, name)(*args)
            msg = bspline.cdll.ddrr_bspline_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            bspline.call(name, *[None if t is _lib._P else 0 for t in argtypes])
    assert bspline.query("ddrr_bspline_workspace_bytes", -1, 30, 37, 4, 5, 3) == -1
    # r1 (3, Dx, Dy, Gz) | r2 (3, Dx, Gy, Gz) floats: 23 x 30 x 37 with (4, 5, 3) -> 3 * 23 * 3 * (30 + 5)
    assert bspline.query("ddrr_bspline_workspace_bytes", 23, 30, 37, 4, 5, 3) == 3 * 23 * 3 * 35 * 4 == 28980
    assert bspline.query("ddrr_bspline_workspace_bytes", 2, 2, 2, 2, 2, 2) == 3 * 2 * 2 * (2 + 2) * 4 == 192


def test_argument_rules(bspline):
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
            (name, _args(name, a, padding=2), "padding"),
            (name, _args(name, a, padding=-1), "padding"),
        ]
    name = "ddrr_bspline_backward_displacement"
    cases += [(name, _args(name, a, ws_bytes=28980 - 1), "ws_bytes"),
              (name, _args(name, a, ws_bytes=-1), "ws_bytes"),
              (name, _args(name, a, ws_off=8194), "4-byte aligned")]
    for name, args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            bspline.call(name, *args)
    # exactly 2^31 voxels is inside the domain (the query launches nothing)
    assert bspline.query("ddrr_bspline_workspace_bytes", 1024, 1024, 2048, 2, 2, 2) == 3 * 1024 * 2 * (1024 + 2) * 4
    # ... also with one node per voxel: r1 and r2 are then three volumes each
    assert bspline.query("ddrr_bspline_workspace_bytes", 1024, 1024, 2048, 1024, 1024, 2048) == 2 * 3 * 2**31 * 4


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_bspline_lib", None)
    monkeypatch.setattr(_lib, "BSPLINE_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_bspline_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops._query_bspline("ddrr_bspline_workspace_bytes", 2, 2, 2, 2, 2, 2)
