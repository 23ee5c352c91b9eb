"""The C ABI of the weighted multi-view Levenberg-Marquardt library: include/diffdrr_wmvlm_hip.h <-> ctypes signatures
<-> libdiffdrr_wmvlm_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_wmvlm_hip.h")
ENTRIES = {"ddrr_wmvlm_abi_version", "ddrr_wmvlm_last_error", "ddrr_wmvlm_workspace_bytes", "ddrr_wmvlm_raygen",
           "ddrr_wmvlm_normal_sums", "ddrr_wmvlm_step"}
OTHERS = ("EXPORTS", "MI_EXPORTS", "RECON_EXPORTS", "FBP_EXPORTS", "LM_EXPORTS", "WARP_EXPORTS", "BSPLINE_EXPORTS",
          "POLYRIGID_EXPORTS", "JACOBIAN_EXPORTS", "PROX_EXPORTS", "WNCC_EXPORTS", "WLM_EXPORTS", "MVLM_EXPORTS")
KERNELS = ("wmv_raygen_kernel", "wmv_normal_sums_kernel", "wmv_step_kernel")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def wmvlm():
    import __graft_entry__ as entry

    entry.build_wmvlm_hip()
    return _lib.wmvlm_library(_lib.WMVLM_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.WMVLM_EXPORTS) == ENTRIES
    for name, argtypes in _lib._WMVLM_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    for other in OTHERS:  # ... and none of it is part of any other library's ABI
        assert not set(decls) & set(getattr(_lib, other)), other
    P, I, F, L, D = _lib._P, _lib._I, _lib._F, _lib._L, _lib._D
    sig = _lib._WMVLM_SIGNATURES
    assert sig["ddrr_wmvlm_workspace_bytes"] == [I, I, I]
    # (ddrr_mvlm_raygen's with P_stride behind P; ddrr_mvlm_normal_sums' with w, w_stride behind x1 and P_stride
    # behind P; ddrr_mvlm_step's without N's use but with sw_views behind ncc_views)
    assert sig["ddrr_wmvlm_raygen"] == [P, P, I, I, I, P, P, P, L, I, I, I, P, P, P, P, P, L, P, P]
    assert sig["ddrr_wmvlm_normal_sums"] == [P, P, P, L, P, P, P, P, L, P, P, I, I, I, P, I, I, I, F, I, P, P, P]
    assert sig["ddrr_wmvlm_step"] == [P, P, P, P, I, I, I, D, D, D, D, D, P, P, P, P]
    assert _lib._WMVLM_RESTYPES == {"ddrr_wmvlm_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_WMVLM_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_WMVLM_ABI_VERSION"]) == _lib.WMVLM_ABI_VERSION == 1
    assert int(const["DDRR_WMVLM_SUMS"]) == _lib.WMVLM_SUMS == _lib.WLM_SUMS == _lib.MVLM_SUMS + 1 == 45
    assert int(const["DDRR_WMVLM_GROUP_RAYS"]) == _lib.WMVLM_GROUP_RAYS == _lib.LM_GROUP_RAYS == 1024
    assert int(const["DDRR_WMVLM_STATE_DOUBLES"]) == _lib.WMVLM_STATE_DOUBLES == _lib.LM_STATE_DOUBLES == 40
    assert int(const["DDRR_WMVLM_MAX_POSES"]) == _lib.WMVLM_MAX_POSES == 65535


def test_the_other_headers_and_their_versions_are_untouched():
    assert _lib.WMVLM_ABI_VERSION == 1 and _lib.WMVLM_HEADER.prefix == "ddrr_wmvlm"
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION, _lib.LM_ABI_VERSION,
            _lib.WARP_ABI_VERSION, _lib.BSPLINE_ABI_VERSION, _lib.POLYRIGID_ABI_VERSION, _lib.JACOBIAN_ABI_VERSION,
            _lib.PROX_ABI_VERSION, _lib.WNCC_ABI_VERSION, _lib.WLM_ABI_VERSION, _lib.MVLM_ABI_VERSION) == (
        33, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    for other in OTHERS:
        assert not any(n.startswith("ddrr_wmvlm") for n in getattr(_lib, other)), other
    assert len(_lib.LM_EXPORTS) == 5 and len(_lib.WLM_EXPORTS) == 5 and len(_lib.MVLM_EXPORTS) == 6
    assert len(_lib.WMVLM_EXPORTS) == 6


def test_the_parent_sources_are_not_part_of_this_library():
    """The library includes the cores of its parents and defines none of their arithmetic again: its sources -- with
    lm_kernels.h, where the kernels' bodies are written once for the four libraries -- name the functions they call
    and hold no second definition of them.  The weighted sums are called through wlm_core.h's WeightedSums, which
    the normal-sums kernel is instantiated on."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    core = open(os.path.join(csrc, "wmvlm_core.h")).read()
    hip = open(os.path.join(csrc, "wmvlm.hip")).read()
    kernels = open(os.path.join(csrc, "lm_kernels.h")).read()
    wlm_core = open(os.path.join(csrc, "wlm_core.h")).read()
    assert '#include "wlm_core.h"' in core and '#include "wmvlm_core.h"' in hip and '#include "lm_kernels.h"' in hip
    assert '#include "lm_core.h"' in wlm_core and '#include "lm_core.h"' in kernels
    assert "normal_sums_body<WeightedSums>(" in hip and "Sums::slice(" in kernels
    assert re.search(r"struct WeightedSums \{[^}]*\bwslice_sum\(", wlm_core)
    for fn in ("ray_jacobian", "wslice_sum", "normal_equations", "judge_and_solve"):
        assert fn + "(" in core + hip + kernels or fn == "wslice_sum", fn
        assert not re.search(r"DDRR_HD\s+[\w:&\s]+\b" + fn + r"\s*\(", core + hip + kernels), fn


def test_library_builds_loads_and_exports_exactly_the_header(wmvlm):
    assert wmvlm.cdll.ddrr_wmvlm_abi_version() == _lib.WMVLM_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.WMVLM_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build_and_the_main_library_does_not_depend_on_the_core():
    import inspect

    import __graft_entry__ as entry

    assert "build_wmvlm_hip()" in inspect.getsource(entry.build)
    assert "wmvlm_library(WMVLM_LIB)" in inspect.getsource(entry.build)
    assert entry.WMVLM_LIB == _lib.WMVLM_LIB_PATH
    assert "wmvlm_core.h" in entry._OWN_HEADERS and "wmvlm_core.h" not in entry.HIP_HEADERS
    assert "wmvlm.hip" not in entry.HIP_SOURCES


def test_library_contains_gfx950_code_object(wmvlm):
    blob = open(_lib.WMVLM_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)


def test_kernels_use_no_scratch_memory(wmvlm):
    """Read the kernel descriptors of the built code object (as tests/test_lm_abi.py does): no private segment in
    any kernel, and at most 128 registers (four waves per SIMD)."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.WMVLM_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_wmvlm.elf")
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
_RAYGEN = ("rot", "xyz", "reorient_v", "Ainv", "P", "Mw", "source_v", "target_v", "img")
_SUMS = ("aux", "x1", "w", "source_v", "Mw", "Ainv", "P", "rot", "xyz", "reorient_v", "ws")


def _raygen_args(a, null=None, S=2, V=2, N=100, axes=(2, 0, 1), clear=0, floats=0, lws=0, P_stride=0):
    p = {n: a + 64 * i for i, n in enumerate(_RAYGEN)}
    if null is not None:
        p[null] = None
    return (p["rot"], p["xyz"], *axes, p["reorient_v"], p["Ainv"], p["P"], P_stride, S, V, N, p["Mw"], p["source_v"],
            p["target_v"], p["img"], clear or None, floats, lws or None, None)


def _sums_args(a, null=None, S=2, V=2, N=100, axes=(2, 0, 1), ws_off=4096, w_stride=0, P_stride=0):
    p = {n: a + 64 * i for i, n in enumerate(_SUMS)}
    p["ws"] = a + ws_off
    if null is not None:
        p[null] = None
    return (p["aux"], p["x1"], p["w"], w_stride, p["source_v"], p["Mw"], p["Ainv"], p["P"], P_stride, p["rot"],
            p["xyz"], *axes, p["reorient_v"], S, V, N, 1e-8, 1, p["ws"], None, None)


def _step_args(a, null=None, S=2, V=2, N=100, eps=1e-5, up=4.0, down=0.25, lo=1e-7, hi=1e6, ws_off=0, views=False,
               sw_off=None):
    ptrs = {"ws": a + ws_off, "state": a + 4096, "rot": a + 8192, "xyz": a + 8256, "ncc_out": a + 8320}
    if null is not None:
        ptrs[null] = None
    return (ptrs["ws"], ptrs["state"], ptrs["rot"], ptrs["xyz"], S, V, N, eps, up, down, lo, hi, ptrs["ncc_out"],
            a + 8384 if views else None, a + 8448 + sw_off if sw_off is not None else None, None)


def _cases(a):
    nan, inf = float("nan"), float("inf")
    cases = [("ddrr_wmvlm_raygen", _raygen_args(a, null=n), "null pointer") for n in _RAYGEN]
    cases += [("ddrr_wmvlm_normal_sums", _sums_args(a, null=n), "null pointer") for n in _SUMS]
    cases += [("ddrr_wmvlm_step", _step_args(a, null=n), "null pointer")
              for n in ("ws", "state", "rot", "xyz", "ncc_out")]
    for entry, make in (("ddrr_wmvlm_raygen", _raygen_args), ("ddrr_wmvlm_normal_sums", _sums_args),
                        ("ddrr_wmvlm_step", _step_args)):
        cases += [
            (entry, make(a, S=-1), "batch"),
            (entry, make(a, V=0), "view count"),
            (entry, make(a, V=-2), "view count"),
            (entry, make(a, N=0), "image size"),
            (entry, make(a, N=-3), "image size"),
            (entry, make(a, S=256, V=256), "65535"),
            (entry, make(a, S=65536, V=1), "65535"),
            (entry, make(a, S=65536, V=65536), "65535"),  # (the product does not wrap)
        ]
    for entry, make in (("ddrr_wmvlm_raygen", _raygen_args), ("ddrr_wmvlm_normal_sums", _sums_args)):
        cases += [(entry, make(a, axes=(0, 0, 1)), "Euler convention"), (entry, make(a, axes=(0, 1, 3)), "Euler convention"),
                  (entry, make(a, axes=(-1, 1, 2)), "Euler convention"),
                  # P_stride is 0 or 3 N
                  (entry, make(a, P_stride=100), "P_stride"), (entry, make(a, P_stride=299), "P_stride"),
                  (entry, make(a, P_stride=-300), "P_stride"), (entry, make(a, P_stride=600), "P_stride")]
    cases += [
        # w_stride is 0 or N
        ("ddrr_wmvlm_normal_sums", _sums_args(a, w_stride=1), "w_stride"),
        ("ddrr_wmvlm_normal_sums", _sums_args(a, w_stride=99), "w_stride"),
        ("ddrr_wmvlm_normal_sums", _sums_args(a, w_stride=-100), "w_stride"),
        ("ddrr_wmvlm_normal_sums", _sums_args(a, w_stride=300), "w_stride"),
        ("ddrr_wmvlm_raygen", _raygen_args(a, floats=8), "clear_floats"),
        ("ddrr_wmvlm_raygen", _raygen_args(a, clear=a + 16384, floats=-1), "clear_floats"),
        ("ddrr_wmvlm_raygen", _raygen_args(a, clear=a + 16388, floats=8), "16-byte aligned"),
        ("ddrr_wmvlm_raygen", _raygen_args(a, lws=a + 16392), "16-byte aligned"),
        ("ddrr_wmvlm_raygen", _raygen_args(a, S=0, clear=a + 16384, floats=8), "empty batch"),
        ("ddrr_wmvlm_raygen", _raygen_args(a, S=0, lws=a + 16384), "empty batch"),
        ("ddrr_wmvlm_normal_sums", _sums_args(a, ws_off=4100), "8-byte aligned"),
        ("ddrr_wmvlm_step", _step_args(a, eps=-1.0), "ncc_eps"),
        ("ddrr_wmvlm_step", _step_args(a, eps=nan), "ncc_eps"),
        ("ddrr_wmvlm_step", _step_args(a, up=1.0), "up must be"),
        ("ddrr_wmvlm_step", _step_args(a, up=inf), "up must be"),
        ("ddrr_wmvlm_step", _step_args(a, down=1.0), "down"),
        ("ddrr_wmvlm_step", _step_args(a, down=0.0), "down"),
        ("ddrr_wmvlm_step", _step_args(a, lo=0.0), "lambda_min"),
        ("ddrr_wmvlm_step", _step_args(a, lo=2.0, hi=1.0), "lambda_min"),
        ("ddrr_wmvlm_step", _step_args(a, hi=inf), "lambda_min"),
        ("ddrr_wmvlm_step", _step_args(a, ws_off=4), "8-byte aligned"),
        ("ddrr_wmvlm_step", _step_args(a, sw_off=4), "8-byte aligned"),
    ]
    return cases


def _no_ops(lib, a):
    """empty batches are valid no-ops (nothing is launched, nothing is written)"""
    assert lib.cdll.ddrr_wmvlm_raygen(*_raygen_args(a, S=0)) == 0
    assert lib.cdll.ddrr_wmvlm_raygen(*_raygen_args(a, S=0, P_stride=300)) == 0
    assert lib.cdll.ddrr_wmvlm_normal_sums(*_sums_args(a, S=0)) == 0
    assert lib.cdll.ddrr_wmvlm_normal_sums(*_sums_args(a, S=0, V=7, w_stride=100, P_stride=300)) == 0
    assert lib.cdll.ddrr_wmvlm_step(*_step_args(a, S=0)) == 0
    assert lib.cdll.ddrr_wmvlm_step(*_step_args(a, S=0, views=True, sw_off=0)) == 0


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(wmvlm):
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._WMVLM_SIGNATURES if n not in _lib._WMVLM_RESTYPES]
    assert status_entries == ["ddrr_wmvlm_raygen", "ddrr_wmvlm_normal_sums", "ddrr_wmvlm_step"]
    for name in status_entries:
        argtypes = _lib._WMVLM_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t in (_lib._I, _lib._L) else 0.5) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(wmvlm.cdll, name)(*args)
            msg = wmvlm.cdll.ddrr_wmvlm_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            wmvlm.call(name, *[None if t is _lib._P else (0 if t in (_lib._I, _lib._L) else 0.5) for t in argtypes])
    q = lambda *a: wmvlm.query("ddrr_wmvlm_workspace_bytes", *a)  # noqa: E731
    assert q(-1, 2, 100) == 0 and q(3, 0, 100) == 0 and q(3, 2, -5) == 0 and q(0, 2, 100) == 0
    assert q(256, 256, 100) == 0 and q(65536, 65536, 100) == 0
    assert q(3, 2, 1024) == 3 * 2 * 45 * 8 and q(3, 2, 1025) == 3 * 2 * 2 * 45 * 8
    assert q(65535, 1, 1) == 65535 * 45 * 8


def test_argument_rules(wmvlm):
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for name, args, what in _cases(a):
        with pytest.raises(RuntimeError, match=what):
            wmvlm.call(name, *args)
    _no_ops(wmvlm, a)


def test_host_build_answers_the_same_rules():
    """tests/emu/wmvlm_emu.cpp validates with the same functions (csrc/wmvlm_core.h)."""
    import wmvlm_cases

    emu = wmvlm_cases.emu_library()
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for name, args, what in _cases(a):
        with pytest.raises(RuntimeError, match=what):
            emu.call(name, *args)
    _no_ops(emu, a)
    assert emu.query("ddrr_wmvlm_workspace_bytes", 3, 2, 1025) == 3 * 2 * 2 * 45 * 8


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_wmvlm_lib", None)
    monkeypatch.setattr(_lib, "WMVLM_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_wmvlm_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops.wmvlm_workspace(1, 2, 10, "cpu")
