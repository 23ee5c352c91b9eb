"""The C ABI of the weighted NCC library: include/diffdrr_wncc_hip.h <-> ctypes signatures <->
libdiffdrr_wncc_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_wncc_hip.h")
ENTRIES = {"ddrr_wncc_abi_version", "ddrr_wncc_last_error", "ddrr_wncc_workspace_bytes", "ddrr_wncc_forward",
           "ddrr_wncc_backward", "ddrr_wncc_siddon_forward", "ddrr_wncc_siddon_backward_pose"}
KERNELS = ("moments_kernelILb0", "moments_kernelILb1", "fold_moments_kernel", "pixel_backward_kernel",
           "siddon_backward_kernel", "fold_pose_kernel")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def wncc():
    import __graft_entry__ as entry

    entry.build_wncc_hip()
    return _lib.wncc_library(_lib.WNCC_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.WNCC_EXPORTS) == ENTRIES
    for name, argtypes in _lib._WNCC_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    for other in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS, _lib.FBP_EXPORTS, _lib.LM_EXPORTS,
                  _lib.WARP_EXPORTS, _lib.BSPLINE_EXPORTS, _lib.POLYRIGID_EXPORTS, _lib.JACOBIAN_EXPORTS,
                  _lib.PROX_EXPORTS):
        assert not set(decls) & set(other)
    P, I, F, L = _lib._P, _lib._I, _lib._F, _lib._L
    sig = _lib._WNCC_SIGNATURES
    assert sig["ddrr_wncc_workspace_bytes"] == [I, I]
    assert sig["ddrr_wncc_forward"] == [P, L, P, P, L, I, I, F, P, P, P, P]
    assert sig["ddrr_wncc_backward"] == [P, L, P, P, L, P, P, I, I, I, P, P, P]
    assert sig["ddrr_wncc_siddon_forward"] == [P, P, P, L, P, L, I, I, F, P, P, P, P, P, P]
    assert sig["ddrr_wncc_siddon_backward_pose"] == [P, P, L, P, L, P, P, I, P, P, P, P, P, P, I, I, I, P, I, I, F, I,
                                                     P, P, P, P]
    assert _lib._WNCC_RESTYPES == {"ddrr_wncc_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_WNCC_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_WNCC_ABI_VERSION"]) == _lib.WNCC_ABI_VERSION == 1
    assert int(const["DDRR_WNCC_GROUP_RAYS"]) == _lib.WNCC_GROUP_RAYS == 1024
    assert int(const["DDRR_WNCC_STATS"]) == _lib.WNCC_STATS == 6
    assert int(const["DDRR_WNCC_SLOT_BYTES"]) == _lib.WNCC_SLOT_BYTES == 6 * 8 == 12 * 4
    assert int(const["DDRR_WNCC_MAX_POSES"]) == _lib.WNCC_MAX_POSES == 65535


def test_the_other_headers_and_their_versions_are_untouched():
    assert _lib.WNCC_ABI_VERSION == 1 and _lib.WNCC_HEADER.prefix == "ddrr_wncc"  # (the eleventh header, next to:)
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION, _lib.LM_ABI_VERSION,
            _lib.WARP_ABI_VERSION, _lib.BSPLINE_ABI_VERSION, _lib.POLYRIGID_ABI_VERSION, _lib.JACOBIAN_ABI_VERSION,
            _lib.PROX_ABI_VERSION) == (33, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    for exports in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS, _lib.FBP_EXPORTS, _lib.LM_EXPORTS,
                    _lib.WARP_EXPORTS, _lib.BSPLINE_EXPORTS, _lib.POLYRIGID_EXPORTS, _lib.JACOBIAN_EXPORTS,
                    _lib.PROX_EXPORTS):
        assert not any(n.startswith("ddrr_wncc") for n in exports)
    assert len(_lib.LM_EXPORTS) == 5 and "ddrr_siddon_ncc_forward" in _lib.EXPORTS


def test_library_builds_loads_and_exports_exactly_the_header(wncc):
    assert wncc.cdll.ddrr_wncc_abi_version() == _lib.WNCC_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.WNCC_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build_and_the_main_library_does_not_depend_on_the_core():
    import inspect

    import __graft_entry__ as entry

    assert "build_wncc_hip()" in inspect.getsource(entry.build)
    assert entry.WNCC_LIB == _lib.WNCC_LIB_PATH
    assert "wncc_core.h" in entry._OWN_HEADERS and "wncc_core.h" not in entry.HIP_HEADERS
    assert "wncc.hip" not in entry.HIP_SOURCES


def test_library_contains_gfx950_code_object(wncc):
    blob = open(_lib.WNCC_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)


def test_kernels_use_no_scratch_memory(wncc):
    """Read the kernel descriptors of the built code object (as tests/test_lm_abi.py does): no private segment in
    any kernel, and at most 128 registers (four waves per SIMD)."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.WNCC_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_wncc.elf")
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
        assert vgpr is not None and vgpr <= 128, (name, vgpr)


# ------------------------------------------------------------------------------------------------ argument rules
def _fwd(a, null=None, B=2, N=100, s1=0, sw=100, eps=1e-5, ws_off=4096):
    p = {"x1": a, "x2": a + 64, "w": a + 128, "ws": a + ws_off, "ncc": a + 192, "stats": a + 256}
    if null:
        p[null] = None
    return (p["x1"], s1, p["x2"], p["w"], sw, B, N, eps, p["ws"], p["ncc"], p["stats"], None)


def _bwd(a, null=None, B=2, N=100, s1=100, sw=0, gs=1, g_x1=True):
    p = {"x1": a, "x2": a + 64, "w": a + 128, "stats": a + 192, "g_out": a + 256}
    if null:
        p[null] = None
    return (p["x1"], s1, p["x2"], p["w"], sw, p["stats"], p["g_out"], gs, B, N, a + 320 if g_x1 else None, a + 384, None)


def _sfwd(a, null=None, B=2, N=100, s1=0, sw=100, eps=1e-5, ws_off=4096):
    p = {"aux": a, "img": a + 64, "x1": a + 128, "w": a + 192, "ws": a + ws_off, "ncc": a + 256, "stats": a + 320}
    if null:
        p[null] = None
    return (p["aux"], p["img"], p["x1"], s1, p["w"], sw, B, N, eps, p["ws"], p["ncc"], p["stats"], None, None, None)


_SBWD = ("aux", "x1", "w", "stats", "g_out", "source_v", "Mw", "Ainv", "P", "rot", "xyz", "reorient34", "ws", "g_rot",
         "g_xyz")


def _sbwd(a, null=None, B=2, N=100, s1=0, sw=100, gs=1, axes=(2, 0, 1), eps=1e-8, ws_off=4096):
    p = {n: a + 64 * i for i, n in enumerate(_SBWD)}
    p["ws"] = a + ws_off
    if null:
        p[null] = None
    return (p["aux"], p["x1"], s1, p["w"], sw, p["stats"], p["g_out"], gs, p["source_v"], p["Mw"], p["Ainv"], p["P"],
            p["rot"], p["xyz"], *axes, p["reorient34"], B, N, eps, 1, p["ws"], p["g_rot"], p["g_xyz"], None)


_ARGS = {"ddrr_wncc_forward": _fwd, "ddrr_wncc_backward": _bwd, "ddrr_wncc_siddon_forward": _sfwd,
         "ddrr_wncc_siddon_backward_pose": _sbwd}


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(wncc):
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._WNCC_SIGNATURES if n not in _lib._WNCC_RESTYPES]
    assert status_entries == list(_ARGS)
    for name in status_entries:
        argtypes = _lib._WNCC_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t in (_lib._I, _lib._L) else 0.5) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(wncc.cdll, name)(*args)
            msg = wncc.cdll.ddrr_wncc_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            wncc.call(name, *[None if t is _lib._P else (0 if t in (_lib._I, _lib._L) else 0.5) for t in argtypes])
    assert wncc.query("ddrr_wncc_workspace_bytes", -1, 100) == 0 and wncc.query("ddrr_wncc_workspace_bytes", 3, -5) == 0
    assert wncc.query("ddrr_wncc_workspace_bytes", 3, 1024) == 3 * 48
    assert wncc.query("ddrr_wncc_workspace_bytes", 3, 1025) == 3 * 2 * 48


def test_argument_rules(wncc):
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    nan, inf = float("nan"), float("inf")
    cases = [("ddrr_wncc_forward", _fwd(a, null=n), "null pointer") for n in ("x1", "x2", "w", "ws", "ncc", "stats")]
    cases += [("ddrr_wncc_backward", _bwd(a, null=n), "null pointer") for n in ("x1", "x2", "w", "stats", "g_out")]
    cases += [("ddrr_wncc_siddon_forward", _sfwd(a, null=n), "null pointer")
              for n in ("aux", "img", "x1", "w", "ws", "ncc", "stats")]
    cases += [("ddrr_wncc_siddon_backward_pose", _sbwd(a, null=n), "null pointer") for n in _SBWD]
    for name, make in _ARGS.items():
        cases += [(name, make(a, B=-1), "batch"), (name, make(a, N=0), "image size"), (name, make(a, N=-3), "image size"),
                  (name, make(a, B=65536), "65535"), (name, make(a, s1=50), "x1_stride"),
                  (name, make(a, sw=50), "w_stride"), (name, make(a, sw=-100), "w_stride")]
        if name != "ddrr_wncc_backward":
            cases += [(name, make(a, ws_off=4100), "8-byte aligned"), (name, make(a, eps=-1.0), "eps"),
                      (name, make(a, eps=nan), "eps"), (name, make(a, eps=inf), "eps")]
        if name in ("ddrr_wncc_backward", "ddrr_wncc_siddon_backward_pose"):
            cases += [(name, make(a, gs=2), "g_stride"), (name, make(a, gs=-1), "g_stride")]
    cases += [("ddrr_wncc_backward", _bwd(a, s1=0), "shared x1"),
              ("ddrr_wncc_siddon_backward_pose", _sbwd(a, axes=(0, 0, 1)), "Euler convention"),
              ("ddrr_wncc_siddon_backward_pose", _sbwd(a, axes=(0, 1, 3)), "Euler convention"),
              ("ddrr_wncc_siddon_backward_pose", _sbwd(a, axes=(-1, 1, 2)), "Euler convention")]
    for name, args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            wncc.call(name, *args)
    # empty batches are valid no-ops (nothing is launched)
    for name, make in _ARGS.items():
        assert getattr(wncc.cdll, name)(*make(a, B=0)) == 0, name
    assert wncc.cdll.ddrr_wncc_backward(*_bwd(a, B=0, s1=0, g_x1=False)) == 0


def test_host_build_answers_the_same_rules():
    """tests/emu/wncc_emu.cpp validates with the same functions (csrc/wncc_core.h)."""
    import wncc_cases

    emu = wncc_cases.emu_library()
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for name, make in _ARGS.items():
        for args, what in ((make(a, N=0), "image size"), (make(a, sw=50), "w_stride")):
            with pytest.raises(RuntimeError, match=what):
                emu.call(name, *args)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_wncc_lib", None)
    monkeypatch.setattr(_lib, "WNCC_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_wncc_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops.wncc_workspace(1, 10, "cpu")
