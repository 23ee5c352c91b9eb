"""The C ABI of the weighted Levenberg-Marquardt library: include/diffdrr_wlm_hip.h <-> ctypes signatures <->
libdiffdrr_wlm_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_wlm_hip.h")
ENTRIES = {"ddrr_wlm_abi_version", "ddrr_wlm_last_error", "ddrr_wlm_workspace_bytes", "ddrr_wlm_normal_sums",
           "ddrr_wlm_step"}
OTHERS = ("EXPORTS", "MI_EXPORTS", "RECON_EXPORTS", "FBP_EXPORTS", "LM_EXPORTS", "WARP_EXPORTS", "BSPLINE_EXPORTS",
          "POLYRIGID_EXPORTS", "JACOBIAN_EXPORTS", "PROX_EXPORTS", "WNCC_EXPORTS")
KERNELS = ("wnormal_sums_kernel", "wstep_kernel")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def wlm():
    import __graft_entry__ as entry

    entry.build_wlm_hip()
    return _lib.wlm_library(_lib.WLM_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.WLM_EXPORTS) == ENTRIES
    for name, argtypes in _lib._WLM_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    for other in OTHERS:  # ... and none of it is part of any other library's ABI
        assert not set(decls) & set(getattr(_lib, other)), other
    P, I, F, L, D = _lib._P, _lib._I, _lib._F, _lib._L, _lib._D
    sig = _lib._WLM_SIGNATURES
    assert sig["ddrr_wlm_workspace_bytes"] == [I, I]
    assert sig["ddrr_wlm_normal_sums"] == [P, P, L, P, L, P, P, P, P, P, P, I, I, I, P, I, I, F, I, P, P, P]
    assert sig["ddrr_wlm_step"] == [P, P, P, P, I, I, D, D, D, D, D, P, P] == _lib._LM_SIGNATURES["ddrr_lm_step"]
    assert _lib._WLM_RESTYPES == {"ddrr_wlm_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_WLM_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_WLM_ABI_VERSION"]) == _lib.WLM_ABI_VERSION == 1
    assert int(const["DDRR_WLM_SUMS"]) == _lib.WLM_SUMS == 45 == _lib.LM_SUMS + 1
    assert int(const["DDRR_WLM_GROUP_RAYS"]) == _lib.WLM_GROUP_RAYS == _lib.LM_GROUP_RAYS == 1024
    assert int(const["DDRR_WLM_STATE_DOUBLES"]) == _lib.WLM_STATE_DOUBLES == _lib.LM_STATE_DOUBLES == 40
    assert int(const["DDRR_WLM_MAX_POSES"]) == _lib.WLM_MAX_POSES == 65535


def test_the_other_headers_and_their_versions_are_untouched():
    assert _lib.WLM_ABI_VERSION == 1 and _lib.WLM_HEADER.prefix == "ddrr_wlm"
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION, _lib.LM_ABI_VERSION,
            _lib.WARP_ABI_VERSION, _lib.BSPLINE_ABI_VERSION, _lib.POLYRIGID_ABI_VERSION, _lib.JACOBIAN_ABI_VERSION,
            _lib.PROX_ABI_VERSION, _lib.WNCC_ABI_VERSION) == (33, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    for other in OTHERS:
        assert not any(n.startswith("ddrr_wlm") for n in getattr(_lib, other)), other
    assert len(_lib.LM_EXPORTS) == 5 and len(_lib.WNCC_EXPORTS) == 7


def test_library_builds_loads_and_exports_exactly_the_header(wlm):
    assert wlm.cdll.ddrr_wlm_abi_version() == _lib.WLM_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.WLM_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build_and_the_main_library_does_not_depend_on_the_core():
    import inspect

    import __graft_entry__ as entry

    assert "build_wlm_hip()" in inspect.getsource(entry.build)
    assert "wlm_library(WLM_LIB)" in inspect.getsource(entry.build)
    assert entry.WLM_LIB == _lib.WLM_LIB_PATH
    assert "wlm_core.h" in entry._OWN_HEADERS and "wlm_core.h" not in entry.HIP_HEADERS
    assert "wlm.hip" not in entry.HIP_SOURCES


def test_library_contains_gfx950_code_object(wlm):
    blob = open(_lib.WLM_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)


def test_kernels_use_no_scratch_memory(wlm):
    """Read the kernel descriptors of the built code object (as tests/test_lm_abi.py does): no private segment in
    either kernel, and at most 128 registers (four waves per SIMD)."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.WLM_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_wlm.elf")
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
_SUMS = ("aux", "x1", "w", "source_v", "Mw", "Ainv", "P", "rot", "xyz", "reorient34", "ws")


def _sums_args(a, null=None, B=2, N=100, axes=(2, 0, 1), s1=0, sw=100, ws_off=4096):
    p = {n: a + 64 * i for i, n in enumerate(_SUMS)}
    p["ws"] = a + ws_off
    if null is not None:
        p[null] = None
    return (p["aux"], p["x1"], s1, p["w"], sw, p["source_v"], p["Mw"], p["Ainv"], p["P"], p["rot"], p["xyz"], *axes,
            p["reorient34"], B, N, 1e-8, 1, p["ws"], None, None)


def _step_args(a, null=None, B=2, N=100, eps=1e-5, up=4.0, down=0.25, lo=1e-7, hi=1e6, ws_off=0):
    ptrs = {"ws": a + ws_off, "state": a + 4096, "rot": a + 8192, "xyz": a + 8256, "ncc_out": a + 8320}
    if null is not None:
        ptrs[null] = None
    return (ptrs["ws"], ptrs["state"], ptrs["rot"], ptrs["xyz"], B, N, eps, up, down, lo, hi, ptrs["ncc_out"], None)


def _cases(a):
    nan, inf = float("nan"), float("inf")
    cases = [("ddrr_wlm_normal_sums", _sums_args(a, null=n), "null pointer") for n in _SUMS]
    cases += [("ddrr_wlm_step", _step_args(a, null=n), "null pointer")
              for n in ("ws", "state", "rot", "xyz", "ncc_out")]
    cases += [
        ("ddrr_wlm_normal_sums", _sums_args(a, B=-1), "batch"),
        ("ddrr_wlm_normal_sums", _sums_args(a, N=0), "image size"),
        ("ddrr_wlm_normal_sums", _sums_args(a, N=-3), "image size"),
        ("ddrr_wlm_normal_sums", _sums_args(a, axes=(0, 0, 1)), "Euler convention"),
        ("ddrr_wlm_normal_sums", _sums_args(a, axes=(0, 1, 3)), "Euler convention"),
        ("ddrr_wlm_normal_sums", _sums_args(a, axes=(-1, 1, 2)), "Euler convention"),
        ("ddrr_wlm_normal_sums", _sums_args(a, s1=50), "x1_stride"),
        ("ddrr_wlm_normal_sums", _sums_args(a, sw=50), "w_stride"),
        ("ddrr_wlm_normal_sums", _sums_args(a, sw=-100), "w_stride"),
        ("ddrr_wlm_normal_sums", _sums_args(a, sw=1), "w_stride"),
        ("ddrr_wlm_normal_sums", _sums_args(a, ws_off=4100), "8-byte aligned"),
        ("ddrr_wlm_normal_sums", _sums_args(a, B=65536), "65535"),
        ("ddrr_wlm_step", _step_args(a, B=-1), "batch"),
        ("ddrr_wlm_step", _step_args(a, N=0), "image size"),
        ("ddrr_wlm_step", _step_args(a, eps=-1.0), "ncc_eps"),
        ("ddrr_wlm_step", _step_args(a, eps=nan), "ncc_eps"),
        ("ddrr_wlm_step", _step_args(a, up=1.0), "up must be"),
        ("ddrr_wlm_step", _step_args(a, up=inf), "up must be"),
        ("ddrr_wlm_step", _step_args(a, down=1.0), "down"),
        ("ddrr_wlm_step", _step_args(a, down=0.0), "down"),
        ("ddrr_wlm_step", _step_args(a, lo=0.0), "lambda_min"),
        ("ddrr_wlm_step", _step_args(a, lo=2.0, hi=1.0), "lambda_min"),
        ("ddrr_wlm_step", _step_args(a, hi=inf), "lambda_min"),
        ("ddrr_wlm_step", _step_args(a, ws_off=4), "8-byte aligned"),
        ("ddrr_wlm_step", _step_args(a, B=65536), "65535"),
    ]
    return cases


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(wlm):
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._WLM_SIGNATURES if n not in _lib._WLM_RESTYPES]
    assert status_entries == ["ddrr_wlm_normal_sums", "ddrr_wlm_step"]
    for name in status_entries:
        argtypes = _lib._WLM_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t in (_lib._I, _lib._L) else 0.5) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(wlm.cdll, name)(*args)
            msg = wlm.cdll.ddrr_wlm_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            wlm.call(name, *[None if t is _lib._P else (0 if t in (_lib._I, _lib._L) else 0.5) for t in argtypes])
    assert wlm.query("ddrr_wlm_workspace_bytes", -1, 100) == 0 and wlm.query("ddrr_wlm_workspace_bytes", 3, -5) == 0
    assert wlm.query("ddrr_wlm_workspace_bytes", 3, 1024) == 3 * 45 * 8
    assert wlm.query("ddrr_wlm_workspace_bytes", 3, 1025) == 3 * 2 * 45 * 8


def test_argument_rules(wlm):
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for name, args, what in _cases(a):
        with pytest.raises(RuntimeError, match=what):
            wlm.call(name, *args)
    # empty batches are valid no-ops (nothing is launched)
    assert wlm.cdll.ddrr_wlm_normal_sums(*_sums_args(a, B=0)) == 0
    assert wlm.cdll.ddrr_wlm_normal_sums(*_sums_args(a, B=0, sw=0, s1=100)) == 0
    assert wlm.cdll.ddrr_wlm_step(*_step_args(a, B=0)) == 0


def test_host_build_answers_the_same_rules():
    """tests/emu/wlm_emu.cpp validates with the same functions (csrc/wlm_core.h)."""
    import wlm_cases

    emu = wlm_cases.emu_library()
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for name, args, what in _cases(a):
        with pytest.raises(RuntimeError, match=what):
            emu.call(name, *args)
    assert emu.cdll.ddrr_wlm_normal_sums(*_sums_args(a, B=0)) == 0 and emu.cdll.ddrr_wlm_step(*_step_args(a, B=0)) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_wlm_lib", None)
    monkeypatch.setattr(_lib, "WLM_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_wlm_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops.wlm_workspace(1, 10, "cpu")
