"""The C ABI of the polyrigid deformation library: include/diffdrr_polyrigid_hip.h <-> ctypes signatures <->
libdiffdrr_polyrigid_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_polyrigid_hip.h")
ENTRIES = {"ddrr_polyrigid_abi_version", "ddrr_polyrigid_last_error", "ddrr_polyrigid_workspace_bytes",
           "ddrr_polyrigid_forward", "ddrr_polyrigid_backward_twists", "ddrr_polyrigid_backward_volume"}
KERNELS = ("forward_kernel", "twist_pieces_kernel", "twist_nodes_kernel", "volume_kernel")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def polyrigid():
    import __graft_entry__ as entry

    entry.build_polyrigid_hip()
    return _lib.polyrigid_library(_lib.POLYRIGID_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.POLYRIGID_EXPORTS) == ENTRIES
    assert all(name.startswith("ddrr_polyrigid_") for name in decls)
    for name, argtypes in _lib._POLYRIGID_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    # ... and none of it is part of the other six libraries' ABIs
    for other in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS, _lib.FBP_EXPORTS, _lib.LM_EXPORTS,
                  _lib.WARP_EXPORTS, _lib.BSPLINE_EXPORTS):
        assert not set(decls) & set(other)
    P, I, L, F = _lib._P, _lib._I, _lib._L, _lib._F
    assert _lib._POLYRIGID_SIGNATURES["ddrr_polyrigid_workspace_bytes"] == [I] * 6
    assert _lib._POLYRIGID_SIGNATURES["ddrr_polyrigid_forward"] == [P, I, I, I, P, I, I, I, F, F, F, I, P, P]
    assert _lib._POLYRIGID_SIGNATURES["ddrr_polyrigid_backward_twists"] == \
        [P, I, I, I, P, I, I, I, F, F, F, I, P, P, L, P, P]
    assert _lib._POLYRIGID_SIGNATURES["ddrr_polyrigid_backward_volume"] == [P, I, I, I, I, I, I, F, F, F, I, P, P, P]
    assert _lib._POLYRIGID_RESTYPES == {"ddrr_polyrigid_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_POLYRIGID_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_POLYRIGID_ABI_VERSION"]) == _lib.POLYRIGID_ABI_VERSION == 1
    assert (int(const["DDRR_POLYRIGID_PADDING_ZEROS"]), int(const["DDRR_POLYRIGID_PADDING_BORDER"])) == \
        (_lib.POLYRIGID_PADDING_ZEROS, _lib.POLYRIGID_PADDING_BORDER) == (0, 1)
    assert int(const["DDRR_POLYRIGID_MAX_DIM"]) == _lib.POLYRIGID_MAX_DIM == 2**16 - 1
    # the pieces are the free-form deformation library's, with six components per node
    assert int(const["DDRR_POLYRIGID_PIECE_VOXELS"]) == _lib.POLYRIGID_PIECE_VOXELS == _lib.WARP_PIECE_VOXELS
    assert int(const["DDRR_POLYRIGID_PIECE_FLOATS"]) == _lib.POLYRIGID_PIECE_FLOATS == 8 * 6
    assert _lib.POLYRIGID_SERIES_TERMS == 8 and _lib.POLYRIGID_SERIES_BELOW == 2.25


def test_the_other_headers_and_their_versions_are_untouched():
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION,
            _lib.LM_ABI_VERSION, _lib.WARP_ABI_VERSION, _lib.BSPLINE_ABI_VERSION) == (33, 1, 1, 1, 1, 1, 1)
    for other in (_lib.EXPORTS, _lib.WARP_EXPORTS, _lib.BSPLINE_EXPORTS):
        assert not any(n.startswith("ddrr_polyrigid") for n in other)


def test_library_builds_loads_and_exports_exactly_the_header(polyrigid):
    assert polyrigid.cdll.ddrr_polyrigid_abi_version() == _lib.POLYRIGID_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.POLYRIGID_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build():
    import inspect

    import __graft_entry__ as entry

    assert "build_polyrigid_hip()" in inspect.getsource(entry.build)
    assert entry.POLYRIGID_LIB == _lib.POLYRIGID_LIB_PATH
    assert "polyrigid_core.h" not in entry.HIP_HEADERS  # (the main library does not rebuild for it)


def test_library_contains_gfx950_code_object(polyrigid):
    blob = open(_lib.POLYRIGID_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)


def test_kernels_use_no_scratch_memory(polyrigid):
    """Read the kernel descriptors of the built code object (as tests/test_warp_abi.py does): no private segment
    in any kernel -- the twist gradient's 48 per-thread sums included -- and at most 168 registers (three waves
    per SIMD), 128 (four) for all but that kernel."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.POLYRIGID_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_polyrigid.elf")
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
        assert scratch == 0, (name, scratch)
        assert vgpr is not None and vgpr <= (168 if "twist_pieces_kernel" in name else 128), (name, vgpr)


def _args(name, a, null=None, D=(23, 30, 37), G=(4, 5, 3), pitch=(0.8, 1.0, 2.5), padding=0, ws_bytes=1 << 20,
          ws_off=8192):
    """Valid host-side arguments of a status entry (nothing is launched for the cases that use them)."""
    ptr = {"V": a, "Xi": a + 64, "W": a + 128, "gW": a + 192, "ws": a + ws_off, "gXi": a + 256, "gV": a + 320}
    if null is not None:
        ptr[null] = None
    if name == "ddrr_polyrigid_forward":
        return (ptr["V"], *D, ptr["Xi"], *G, *pitch, padding, ptr["W"], None)
    if name == "ddrr_polyrigid_backward_twists":
        return (ptr["V"], *D, ptr["Xi"], *G, *pitch, padding, ptr["gW"], ptr["ws"], ws_bytes, ptr["gXi"], None)
    return (ptr["Xi"], *G, *D, *pitch, padding, ptr["gW"], ptr["gV"], None)


POINTERS = {"ddrr_polyrigid_forward": ("V", "Xi", "W"),
            "ddrr_polyrigid_backward_twists": ("V", "Xi", "gW", "ws", "gXi"),
            "ddrr_polyrigid_backward_volume": ("Xi", "gW", "gV")}


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(polyrigid):
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._POLYRIGID_SIGNATURES if n not in _lib._POLYRIGID_RESTYPES]
    assert status_entries == list(POINTERS)
    for name in status_entries:
        argtypes = _lib._POLYRIGID_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (1.0 if t is _lib._F else ints) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(polyrigid.cdll, name)(*args)
            msg = polyrigid.cdll.ddrr_polyrigid_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            polyrigid.call(name, *[None if t is _lib._P else 0 for t in argtypes])
    assert polyrigid.query("ddrr_polyrigid_workspace_bytes", -1, 30, 37, 4, 5, 3) == -1
    # 23 x 30 x 37 with (4, 5, 3): cells of at most 8 x 8 x 18 voxels = 2 pieces, 3 * 4 * 2 cells
    assert polyrigid.query("ddrr_polyrigid_workspace_bytes", 23, 30, 37, 4, 5, 3) == 24 * 2 * 48 * 4
    assert polyrigid.query("ddrr_polyrigid_workspace_bytes", 2, 2, 2, 2, 2, 2) == 48 * 4


def test_argument_rules(polyrigid):
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    cases = [(name, _args(name, a, null=n), "null pointer") for name, ptrs in POINTERS.items() for n in ptrs]
    for name in POINTERS:
        cases += [
            (name, _args(name, a, D=(23, -30, 37)), "positive"),
            (name, _args(name, a, D=(0, 30, 37)), "positive"),
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
            (name, _args(name, a, pitch=(0.8, 0.0, 2.5)), "pitch"),
            (name, _args(name, a, pitch=(-0.8, 1.0, 2.5)), "pitch"),
            (name, _args(name, a, pitch=(0.8, 1.0, float("inf"))), "pitch"),
            (name, _args(name, a, pitch=(float("nan"), 1.0, 2.5)), "pitch"),
        ]
    name = "ddrr_polyrigid_backward_twists"
    cases += [(name, _args(name, a, ws_bytes=24 * 2 * 48 * 4 - 1), "ws_bytes"),
              (name, _args(name, a, ws_bytes=-1), "ws_bytes"),
              (name, _args(name, a, ws_off=8194), "4-byte aligned")]
    for name, args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            polyrigid.call(name, *args)
    # the workspace query outside the domain
    for D, G in (((23, 30, 37), (4, 5, 1)), ((23, 30, 37), (4, 31, 3)), ((65536, 2, 2), (2, 2, 2)),
                 ((2048, 2048, 513), (2, 2, 2)), ((0, 30, 37), (4, 5, 3))):
        assert polyrigid.query("ddrr_polyrigid_workspace_bytes", *D, *G) == -1
        assert polyrigid.cdll.ddrr_polyrigid_last_error()
    # exactly 2^31 voxels is inside the domain (the query launches nothing)
    assert polyrigid.query("ddrr_polyrigid_workspace_bytes", 1024, 1024, 2048, 2, 2, 2) == (2**31 // 1024) * 48 * 4
    # ... also with one node per voxel: cells of at most 2 x 2 x 2 voxels, one piece each
    assert polyrigid.query("ddrr_polyrigid_workspace_bytes", 1024, 1024, 2048, 1024, 1024, 2048) == \
        1023 * 1023 * 2047 * 48 * 4


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_polyrigid_lib", None)
    monkeypatch.setattr(_lib, "POLYRIGID_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_polyrigid_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops._query_polyrigid("ddrr_polyrigid_workspace_bytes", 2, 2, 2, 2, 2, 2)
