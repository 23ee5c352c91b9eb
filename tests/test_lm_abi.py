"""The C ABI of the Levenberg-Marquardt library: include/diffdrr_lm_hip.h <-> ctypes signatures <->
libdiffdrr_lm_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_lm_hip.h")
ENTRIES = {"ddrr_lm_abi_version", "ddrr_lm_last_error", "ddrr_lm_workspace_bytes", "ddrr_lm_normal_sums",
           "ddrr_lm_step"}


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def lm():
    import __graft_entry__ as entry

    entry.build_lm_hip()
    return _lib.lm_library(_lib.LM_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.LM_EXPORTS) == ENTRIES
    for name, argtypes in _lib._LM_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    # ... and none of it is part of the other four libraries' ABIs
    for other in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS, _lib.FBP_EXPORTS):
        assert not set(decls) & set(other)
    P, I, F, L, D = _lib._P, _lib._I, _lib._F, _lib._L, _lib._D
    assert _lib._LM_SIGNATURES["ddrr_lm_workspace_bytes"] == [I, I]
    assert _lib._LM_SIGNATURES["ddrr_lm_normal_sums"] == [P, P, L, P, P, P, P, P, P, I, I, I, P, I, I, F, I, P, P, P]
    assert _lib._LM_SIGNATURES["ddrr_lm_step"] == [P, P, P, P, I, I, D, D, D, D, D, P, P]
    assert _lib._LM_RESTYPES == {"ddrr_lm_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_LM_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_LM_ABI_VERSION"]) == _lib.LM_ABI_VERSION == 1
    assert int(const["DDRR_LM_SUMS"]) == _lib.LM_SUMS == 44 == 21 + 3 * 6 + 5
    assert int(const["DDRR_LM_GROUP_RAYS"]) == _lib.LM_GROUP_RAYS == 1024
    assert int(const["DDRR_LM_STATE_DOUBLES"]) == _lib.LM_STATE_DOUBLES == 40
    assert int(const["DDRR_LM_MAX_POSES"]) == _lib.LM_MAX_POSES == 65535


def test_the_other_headers_and_their_versions_are_untouched():
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION) == (33, 1, 1, 1)
    assert not any(n.startswith("ddrr_lm") for n in _lib.EXPORTS)


def test_library_builds_loads_and_exports_exactly_the_header(lm):
    assert lm.cdll.ddrr_lm_abi_version() == _lib.LM_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LM_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build():
    import inspect

    import __graft_entry__ as entry

    assert "build_lm_hip()" in inspect.getsource(entry.build)
    assert entry.LM_LIB == _lib.LM_LIB_PATH


def test_the_kernel_bodies_of_the_four_libraries_are_written_once():
    """The record loads, the pose prologue of the sums and the pose of the ray generation are called in exactly one
    of the four libraries' sources and lm_kernels.h: the bodies are shared, not copied."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    files = ("lm.hip", "wlm.hip", "mvlm.hip", "wmvlm.hip", "lm_kernels.h")
    text = {f: open(os.path.join(csrc, f)).read() for f in files}
    for call in ("rec_blocked_load(", "pose_euler_adjoint_setup(", "pose_euler_forward("):
        assert [f for f in files if call in text[f]] == ["lm_kernels.h"], call


def test_library_contains_gfx950_code_object(lm):
    blob = open(_lib.LM_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"normal_sums_kernel" in blob and b"step_kernel" in blob


def test_kernels_use_no_scratch_memory(lm):
    """Read the kernel descriptors of the built code object (as tests/test_fbp_abi.py does): no private
    segment in any kernel, and at most 128 registers (four waves per SIMD)."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.LM_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_lm.elf")
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
    assert sum("normal_sums_kernel" in k for k in kernels) == 1, sorted(kernels)
    assert sum("step_kernel" in k for k in kernels) == 1, sorted(kernels)
    assert len(kernels) == 2, sorted(kernels)
    for name, (scratch, vgpr) in kernels.items():
        assert scratch == 0, (name, scratch)
        assert vgpr is not None and vgpr <= 128, (name, vgpr)


def _sums_args(a, null=None, B=2, N=100, axes=(2, 0, 1), stride=0, ws_off=4096):
    ptrs = [a + 64 * i for i in range(10)]  # aux x1 source Mw Ainv P rot xyz reorient ws
    names = ["aux", "x1", "source_v", "Mw", "Ainv", "P", "rot", "xyz", "reorient34", "ws"]
    ptrs[9] = a + ws_off
    if null is not None:
        ptrs[names.index(null)] = None
    aux, x1, src, Mw, Ainv, P, rot, xyz, Ro, ws = ptrs
    return (aux, x1, stride, src, Mw, Ainv, P, rot, xyz, *axes, Ro, B, N, 1e-8, 1, ws, None, None)


def _step_args(a, null=None, B=2, N=100, eps=1e-5, up=4.0, down=0.25, lo=1e-7, hi=1e6, ws_off=0):
    ptrs = {"ws": a + ws_off, "state": a + 4096, "rot": a + 8192, "xyz": a + 8256, "ncc_out": a + 8320}
    if null is not None:
        ptrs[null] = None
    return (ptrs["ws"], ptrs["state"], ptrs["rot"], ptrs["xyz"], B, N, eps, up, down, lo, hi, ptrs["ncc_out"], None)


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(lm):
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._LM_SIGNATURES if n not in _lib._LM_RESTYPES]
    assert status_entries == ["ddrr_lm_normal_sums", "ddrr_lm_step"]
    for name in status_entries:
        argtypes = _lib._LM_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t in (_lib._I, _lib._L) else 0.5) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(lm.cdll, name)(*args)
            msg = lm.cdll.ddrr_lm_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            lm.call(name, *[None if t is _lib._P else (0 if t in (_lib._I, _lib._L) else 0.5) for t in argtypes])
    assert lm.query("ddrr_lm_workspace_bytes", -1, 100) == 0 and lm.query("ddrr_lm_workspace_bytes", 3, -5) == 0
    assert lm.query("ddrr_lm_workspace_bytes", 3, 1024) == 3 * 44 * 8
    assert lm.query("ddrr_lm_workspace_bytes", 3, 1025) == 3 * 2 * 44 * 8


def test_argument_rules(lm):
    buf = (ctypes.c_char * 32768)()
    a = (ctypes.addressof(buf) + 15) & ~15
    nan, inf = float("nan"), float("inf")
    cases = [("ddrr_lm_normal_sums", _sums_args(a, null=n), "null pointer")
             for n in ("aux", "x1", "source_v", "Mw", "Ainv", "P", "rot", "xyz", "reorient34", "ws")]
    cases += [("ddrr_lm_step", _step_args(a, null=n), "null pointer") for n in ("ws", "state", "rot", "xyz", "ncc_out")]
    cases += [
        ("ddrr_lm_normal_sums", _sums_args(a, B=-1), "batch"),
        ("ddrr_lm_normal_sums", _sums_args(a, N=0), "image size"),
        ("ddrr_lm_normal_sums", _sums_args(a, N=-3), "image size"),
        ("ddrr_lm_normal_sums", _sums_args(a, axes=(0, 0, 1)), "Euler convention"),
        ("ddrr_lm_normal_sums", _sums_args(a, axes=(0, 1, 3)), "Euler convention"),
        ("ddrr_lm_normal_sums", _sums_args(a, axes=(-1, 1, 2)), "Euler convention"),
        ("ddrr_lm_normal_sums", _sums_args(a, stride=50), "x1_stride"),
        ("ddrr_lm_normal_sums", _sums_args(a, ws_off=4100), "8-byte aligned"),
        ("ddrr_lm_normal_sums", _sums_args(a, B=65536), "65535"),
        ("ddrr_lm_step", _step_args(a, B=-1), "batch"),
        ("ddrr_lm_step", _step_args(a, N=0), "image size"),
        ("ddrr_lm_step", _step_args(a, eps=-1.0), "ncc_eps"),
        ("ddrr_lm_step", _step_args(a, eps=nan), "ncc_eps"),
        ("ddrr_lm_step", _step_args(a, up=1.0), "up must be"),
        ("ddrr_lm_step", _step_args(a, up=inf), "up must be"),
        ("ddrr_lm_step", _step_args(a, down=1.0), "down"),
        ("ddrr_lm_step", _step_args(a, down=0.0), "down"),
        ("ddrr_lm_step", _step_args(a, lo=0.0), "lambda_min"),
        ("ddrr_lm_step", _step_args(a, lo=2.0, hi=1.0), "lambda_min"),
        ("ddrr_lm_step", _step_args(a, hi=inf), "lambda_min"),
        ("ddrr_lm_step", _step_args(a, ws_off=4), "8-byte aligned"),
        ("ddrr_lm_step", _step_args(a, B=65536), "65535"),
    ]
    for name, args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            lm.call(name, *args)
    # empty batches are valid no-ops (nothing is launched)
    assert lm.cdll.ddrr_lm_normal_sums(*_sums_args(a, B=0)) == 0
    assert lm.cdll.ddrr_lm_step(*_step_args(a, B=0)) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lm_lib", None)
    monkeypatch.setattr(_lib, "LM_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_lm_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops.lm_workspace(1, 10, "cpu")
