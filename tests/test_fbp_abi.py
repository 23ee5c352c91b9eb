"""The C ABI of the FDK library: include/diffdrr_fbp_hip.h <-> ctypes signatures <-> libdiffdrr_fbp_hip.so.
No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_fbp_hip.h")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def fbp():
    import __graft_entry__ as entry

    entry.build_fbp_hip()
    return _lib.fbp_library(_lib.FBP_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.FBP_EXPORTS) == {
        "ddrr_fbp_abi_version", "ddrr_fbp_last_error", "ddrr_fbp_filter", "ddrr_fbp_backproject"}
    for name, argtypes in _lib._FBP_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    # ... and none of it is part of the other three libraries' ABIs
    for other in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS):
        assert not set(decls) & set(other)
    P, I, F = _lib._P, _lib._I, _lib._F
    assert _lib._FBP_SIGNATURES["ddrr_fbp_filter"] == [P, I, I, I, I, P, F, F, F, F, F, F, I, P, P]
    assert _lib._FBP_SIGNATURES["ddrr_fbp_backproject"] == [P, I, I, I, P, I, P, I, I, I, I, P]
    assert _lib._FBP_RESTYPES == {}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_FBP_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_FBP_ABI_VERSION"]) == _lib.FBP_ABI_VERSION == 1
    assert int(const["DDRR_FBP_MAX_IMAGE_DIM"]) == _lib.FBP_MAX_IMAGE_DIM == 4096
    assert int(const["DDRR_FBP_MAX_VIEWS"]) == _lib.FBP_MAX_VIEWS == 65535
    assert int(const["DDRR_FBP_MAX_DIM"]) == _lib.FBP_MAX_DIM == 65535
    assert int(const["DDRR_FBP_VIEW_FLOATS"]) == _lib.FBP_VIEW_FLOATS == 16


def test_library_builds_loads_and_exports_exactly_the_header(fbp):
    assert fbp.cdll.ddrr_fbp_abi_version() == _lib.FBP_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.FBP_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_library_contains_gfx950_code_object(fbp):
    blob = open(_lib.FBP_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"filter_kernel" in blob and b"backproject_kernel" in blob


def test_kernels_use_no_scratch_memory(fbp):
    """Read the kernel descriptors of the built code object (as tests/test_recon_abi.py does): no private
    segment in any kernel, and registers for two or more 256-thread workgroups per SIMD."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.FBP_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_fbp.elf")
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
    assert sum("filter_kernel" in k for k in kernels) == 2, sorted(kernels)  # one per axis
    assert sum("backproject_kernel" in k for k in kernels) == 1, sorted(kernels)
    assert len(kernels) == 3, sorted(kernels)
    for name, (scratch, vgpr) in kernels.items():
        assert scratch == 0, (name, scratch)
        assert vgpr is not None and vgpr <= 128, (name, vgpr)


def _filter_args(a, images="a", dims=(2, 4, 4), axis=0, taps="a", scale=1.0, geo=(0.0, 1.0, 0.0, 1.0, 100.0), cw=1,
                 out="a"):
    pick = lambda p, off: a + off if p == "a" else p  # noqa: E731
    return (pick(images, 0), *dims, axis, pick(taps, 4096), scale, *geo, cw, pick(out, 2048), None)


def _bp_args(a, images="a", dims=(2, 4, 4), views="a", dw=1, volume="a", vdims=(4, 4, 4), accumulate=0):
    pick = lambda p, off: a + off if p == "a" else p  # noqa: E731
    return (pick(images, 0), *dims, pick(views, 4096), dw, pick(volume, 2048), *vdims, accumulate, None)


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(fbp):
    buf = (ctypes.c_char * 8192)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._FBP_SIGNATURES if n not in _lib._FBP_RESTYPES]
    assert status_entries == ["ddrr_fbp_filter", "ddrr_fbp_backproject"]
    for name in status_entries:
        argtypes = _lib._FBP_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t is _lib._I else 0.5) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(fbp.cdll, name)(*args)
            msg = fbp.cdll.ddrr_fbp_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            fbp.call(name, *[None if t is _lib._P else (0 if t is _lib._I else 0.5) for t in argtypes])


def test_argument_rules(fbp):
    buf = (ctypes.c_char * 16384)()
    a = (ctypes.addressof(buf) + 15) & ~15
    nan, inf = float("nan"), float("inf")
    for name, args, what in (
            ("ddrr_fbp_filter", _filter_args(a, images=None), "null images"),
            ("ddrr_fbp_filter", _filter_args(a, taps=None), "null taps"),
            ("ddrr_fbp_filter", _filter_args(a, out=None), "null out"),
            ("ddrr_fbp_filter", _filter_args(a, dims=(-1, 4, 4)), "B, H, W"),
            ("ddrr_fbp_filter", _filter_args(a, dims=(2, -4, 4)), "B, H, W"),
            ("ddrr_fbp_filter", _filter_args(a, dims=(2, 4, -4)), "B, H, W"),
            ("ddrr_fbp_filter", _filter_args(a, dims=(1, 4097, 4)), "4096"),
            ("ddrr_fbp_filter", _filter_args(a, dims=(1, 4, 4097)), "4096"),
            ("ddrr_fbp_filter", _filter_args(a, dims=(129, 4096, 4096)), r"2\^31"),
            ("ddrr_fbp_filter", _filter_args(a, axis=2), "axis"),
            ("ddrr_fbp_filter", _filter_args(a, axis=-1), "axis"),
            ("ddrr_fbp_filter", _filter_args(a, scale=nan), "scale"),
            ("ddrr_fbp_filter", _filter_args(a, geo=(0.0, 1.0, 0.0, 1.0, 0.0)), "sdd"),
            ("ddrr_fbp_filter", _filter_args(a, geo=(0.0, inf, 0.0, 1.0, 100.0)), "finite"),
            ("ddrr_fbp_filter", _filter_args(a, geo=(nan, 1.0, 0.0, 1.0, 100.0)), "finite"),
            ("ddrr_fbp_filter", _filter_args(a, out=a + 64), "overlap"),
            ("ddrr_fbp_filter", _filter_args(a, out=a), "overlap"),
            ("ddrr_fbp_filter", _filter_args(a, images=a + 2), "4-byte aligned"),
            ("ddrr_fbp_filter", _filter_args(a, out=a + 2050), "4-byte aligned"),
            ("ddrr_fbp_backproject", _bp_args(a, images=None), "null images"),
            ("ddrr_fbp_backproject", _bp_args(a, views=None), "null views"),
            ("ddrr_fbp_backproject", _bp_args(a, volume=None), "null volume"),
            ("ddrr_fbp_backproject", _bp_args(a, dims=(-1, 4, 4)), "B, H, W"),
            ("ddrr_fbp_backproject", _bp_args(a, dims=(1, 4097, 4)), "4096"),
            ("ddrr_fbp_backproject", _bp_args(a, dims=(1, 4, 4097)), "4096"),
            ("ddrr_fbp_backproject", _bp_args(a, dims=(65536, 1, 1)), "65535"),
            ("ddrr_fbp_backproject", _bp_args(a, vdims=(4, -1, 4)), "Dx, Dy, Dz"),
            ("ddrr_fbp_backproject", _bp_args(a, vdims=(4, 4, 65536)), "65535"),
            ("ddrr_fbp_backproject", _bp_args(a, vdims=(4096, 4096, 2048)), r"2\^34"),
            ("ddrr_fbp_backproject", _bp_args(a, volume=a + 64), "overlap"),
            ("ddrr_fbp_backproject", _bp_args(a, volume=a + 2), "4-byte aligned"),
            ("ddrr_fbp_backproject", _bp_args(a, views=a + 4098), "4-byte aligned")):
        with pytest.raises(RuntimeError, match=what):
            fbp.call(name, *args)
    # empty inputs are valid no-ops (nothing is launched)
    assert fbp.cdll.ddrr_fbp_filter(*_filter_args(a, dims=(0, 4, 4))) == 0
    assert fbp.cdll.ddrr_fbp_filter(*_filter_args(a, dims=(2, 0, 4))) == 0
    assert fbp.cdll.ddrr_fbp_filter(*_filter_args(a, dims=(2, 4, 0), axis=1)) == 0
    assert fbp.cdll.ddrr_fbp_backproject(*_bp_args(a, vdims=(0, 4, 4))) == 0
    assert fbp.cdll.ddrr_fbp_backproject(*_bp_args(a, vdims=(4, 4, 0), accumulate=1)) == 0
    assert fbp.cdll.ddrr_fbp_backproject(*_bp_args(a, dims=(0, 4, 4), accumulate=1)) == 0  # adding nothing


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_fbp_lib", None)
    monkeypatch.setattr(_lib, "FBP_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_fbp_lib()
