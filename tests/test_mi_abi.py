"""The C ABI of the MutualInformation library: include/diffdrr_mi_hip.h <-> ctypes signatures <->
libdiffdrr_mi_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_mi_hip.h")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def mi():
    import __graft_entry__ as entry

    entry.build_mi_hip()
    return _lib.mi_library(_lib.MI_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.MI_EXPORTS)
    for name, argtypes in _lib._MI_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    # ... and none of it is part of the main library's ABI
    assert not set(decls) & set(_lib.EXPORTS)


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_MI_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_MI_ABI_VERSION"]) == _lib.MI_ABI_VERSION
    assert int(const["DDRR_MI_MAX_BINS"]) == _lib.MI_MAX_BINS == 256


def test_library_builds_loads_and_exports_exactly_the_header(mi):
    assert mi.cdll.ddrr_mi_abi_version() == _lib.MI_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.MI_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_library_contains_gfx950_code_object(mi):
    blob = open(_lib.MI_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"mi_joint_kernel" in blob and b"mi_grad_kernel" in blob


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(mi):
    buf = (ctypes.c_char * 4096)()
    addr = ctypes.addressof(buf)
    status_entries = [n for n in _lib._MI_SIGNATURES if n not in _lib._MI_RESTYPES]
    assert status_entries == ["ddrr_mi_forward", "ddrr_mi_backward"]
    for name in status_entries:
        argtypes = _lib._MI_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t in (_lib._I, _lib._L) else 0.0) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(mi.cdll, name)(*args)
            msg = mi.cdll.ddrr_mi_last_error().decode(errors="replace")
            assert rc < 0 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            mi.call(name, *[None if t is _lib._P else (0 if t in (_lib._I, _lib._L) else 0.0) for t in argtypes])
    # the size queries: -1 for invalid sizes
    assert mi.query("ddrr_mi_workspace_bytes", -1, 4, 4, 8) == -1
    assert mi.query("ddrr_mi_workspace_bytes", 1, 0, 4, 8) == -1
    assert mi.query("ddrr_mi_workspace_bytes", 1, 4, 4, 257) == -1
    assert mi.query("ddrr_mi_workspace_bytes", 0, 4, 4, 8) == 0
    assert mi.query("ddrr_mi_workspace_bytes", 8, 256, 256, 256) < 64 * 2**20
    assert mi.query("ddrr_mi_state_floats", 0) == -1
    assert mi.query("ddrr_mi_state_floats", 256) == 256 * 256 + 2 * 256


def test_argument_rules(mi):
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    ws = 1 << 20

    def fwd(K=8, eps=1e-10, bins=a, sigma=a, B=1, s1=16, ws_bytes=ws):
        return (a, s1, a, 16, B, 4, 4, bins, K, sigma, eps, 1, a, ws_bytes, a, None, None)

    def bwd(K=8, bins=a, sigma=a, which=1, g_stride=1):
        return (a, 16, a, 16, 1, 4, 4, bins, K, sigma, a, which, a, g_stride, a, None)

    for name, args, what in (
            ("ddrr_mi_forward", fwd(K=0), "num_bins"),
            ("ddrr_mi_forward", fwd(K=257), "num_bins"),
            ("ddrr_mi_forward", fwd(eps=-1.0), "epsilon"),
            ("ddrr_mi_forward", fwd(eps=float("nan")), "epsilon"),
            ("ddrr_mi_forward", fwd(sigma=None), "null sigma"),
            ("ddrr_mi_forward", fwd(bins=None), "null bins"),
            ("ddrr_mi_forward", fwd(s1=5), "x1_stride"),
            ("ddrr_mi_forward", fwd(ws_bytes=16), "workspace_bytes"),
            ("ddrr_mi_backward", bwd(K=0), "num_bins"),
            ("ddrr_mi_backward", bwd(K=300), "num_bins"),
            ("ddrr_mi_backward", bwd(sigma=None), "null sigma"),
            ("ddrr_mi_backward", bwd(bins=None), "null bins"),
            ("ddrr_mi_backward", bwd(which=2), "which"),
            ("ddrr_mi_backward", bwd(g_stride=3), "g_stride")):
        with pytest.raises(RuntimeError, match=what):
            mi.call(name, *args)
    # an empty batch is a valid no-op (nothing is launched)
    assert mi.cdll.ddrr_mi_forward(*fwd(B=0)) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_mi_lib", None)
    monkeypatch.setattr(_lib, "MI_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_mi_lib()
