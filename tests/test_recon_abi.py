"""The C ABI of the reconstruction library: include/diffdrr_recon_hip.h <-> ctypes signatures <->
libdiffdrr_recon_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_recon_hip.h")
INF = float("inf")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def recon():
    import __graft_entry__ as entry

    entry.build_recon_hip()
    return _lib.recon_library(_lib.RECON_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.RECON_EXPORTS) == {
        "ddrr_recon_abi_version", "ddrr_recon_last_error", "ddrr_recon_tv_workspace_bytes", "ddrr_recon_tv3d",
        "ddrr_recon_adam_step"}
    for name, argtypes in _lib._RECON_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    # ... and none of it is part of the other libraries' ABIs
    assert not set(decls) & set(_lib.EXPORTS) and not set(decls) & set(_lib.MI_EXPORTS)
    # the types the binding derived: doubles for Adam's hyper-parameters, a long element count
    adam = _lib._RECON_SIGNATURES["ddrr_recon_adam_step"]
    assert adam == [_lib._P] * 5 + [_lib._L] + [_lib._D] * 4 + [_lib._F] * 2 + [_lib._I, _lib._P]
    assert _lib._RECON_RESTYPES == {"ddrr_recon_tv_workspace_bytes": _lib._L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_RECON_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_RECON_ABI_VERSION"]) == _lib.RECON_ABI_VERSION
    assert int(const["DDRR_RECON_TV_ISOTROPIC"]) == _lib.RECON_TV_ISOTROPIC == 0
    assert int(const["DDRR_RECON_TV_ANISOTROPIC"]) == _lib.RECON_TV_ANISOTROPIC == 1
    assert int(const["DDRR_RECON_MAX_DIM"]) == _lib.RECON_MAX_DIM == 65535


def test_library_builds_loads_and_exports_exactly_the_header(recon):
    assert recon.cdll.ddrr_recon_abi_version() == _lib.RECON_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.RECON_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_library_contains_gfx950_code_object(recon):
    blob = open(_lib.RECON_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"tv3d_kernel" in blob and b"tv3d_sum_kernel" in blob and b"adam_kernel" in blob


def test_kernels_use_no_scratch_memory(recon):
    """A streaming stencil that spills is a slow one, silently: read the kernel descriptors of the built
    code object (as tests/test_abi.py does for the brick kernels) -- no private segment in any kernel."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.RECON_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_recon.elf")
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
    tv = [k for k in kernels if "tv3d_kernel" in k]
    assert len(tv) == 6, sorted(kernels)  # two modes x three call forms
    assert sum("adam_kernel" in k for k in kernels) == 2, sorted(kernels)
    for name, (scratch, vgpr) in kernels.items():
        assert scratch == 0, (name, scratch)
        assert vgpr is not None and vgpr <= 128, (name, vgpr)  # (256-thread workgroups: two or more per SIMD)


def _tv_args(a, vol="a", dims=(4, 4, 4), spacing=(1.0, 1.0, 1.0), mode=0, eps=1e-3, grad=None, weight=1.0,
             scale=None, ws="a", ws_bytes=1 << 20, value="a"):
    pick = lambda p: a if p == "a" else p  # noqa: E731
    return (pick(vol), *dims, *spacing, mode, eps, grad, 0, weight, scale, pick(ws), ws_bytes, pick(value), None)


def _adam_args(a, p="a", g="a", m="a", v="a", step="a", n=4, lr=0.1, b1=0.9, b2=0.999, eps=1e-8, lower=-INF,
               upper=INF):
    pick = lambda x, off: a + off if x == "a" else x  # noqa: E731
    return (pick(p, 0), pick(g, 256), pick(m, 512), pick(v, 768), pick(step, 1024), n, lr, b1, b2, eps, lower,
            upper, 0, None)


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(recon):
    buf = (ctypes.c_char * 8192)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._RECON_SIGNATURES if n not in _lib._RECON_RESTYPES]
    assert status_entries == ["ddrr_recon_tv3d", "ddrr_recon_adam_step"]
    for name in status_entries:
        argtypes = _lib._RECON_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t in (_lib._I, _lib._L) else 0.5) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(recon.cdll, name)(*args)
            msg = recon.cdll.ddrr_recon_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            recon.call(name, *[None if t is _lib._P else (0 if t in (_lib._I, _lib._L) else 0.5) for t in argtypes])
    # the size query: -1 for invalid sizes, 0 for an empty volume, small for the largest volumes
    q = lambda *d: recon.query("ddrr_recon_tv_workspace_bytes", *d)  # noqa: E731
    assert q(-1, 4, 4) == -1 and q(4, 65536, 4) == -1 and q(4096, 4096, 4096) == -1
    assert q(0, 4, 4) == 0 and q(4, 4, 0) == 0
    assert q(1, 1, 1) == 8
    assert q(512, 512, 512) == 8 * (512 // 32) * (512 // 16) * (512 // 64)
    assert 0 < q(2048, 2048, 4096) <= 8 * 2**20  # 2^34 voxels
    assert 0 < q(65535, 65535, 4) <= 128 * 2**20


def test_argument_rules(recon):
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 15) & ~15
    nan = float("nan")
    for name, args, what in (
            ("ddrr_recon_tv3d", _tv_args(a, vol=None), "null volume"),
            ("ddrr_recon_tv3d", _tv_args(a, ws=None), "null workspace"),
            ("ddrr_recon_tv3d", _tv_args(a, value=None), "null value"),
            ("ddrr_recon_tv3d", _tv_args(a, dims=(4, -1, 4)), "Dx, Dy, Dz"),
            ("ddrr_recon_tv3d", _tv_args(a, dims=(4, 4, 65536)), "65535"),
            ("ddrr_recon_tv3d", _tv_args(a, dims=(4096, 4096, 2048)), r"2\^34"),
            ("ddrr_recon_tv3d", _tv_args(a, spacing=(1.0, 0.0, 1.0)), "sx, sy, sz"),
            ("ddrr_recon_tv3d", _tv_args(a, spacing=(1.0, 1.0, INF)), "sx, sy, sz"),
            ("ddrr_recon_tv3d", _tv_args(a, spacing=(nan, 1.0, 1.0)), "sx, sy, sz"),
            ("ddrr_recon_tv3d", _tv_args(a, mode=2), "mode"),
            ("ddrr_recon_tv3d", _tv_args(a, eps=-1.0), "eps"),
            ("ddrr_recon_tv3d", _tv_args(a, eps=nan), "eps"),
            ("ddrr_recon_tv3d", _tv_args(a, grad=a + 4096, weight=nan), "weight"),
            ("ddrr_recon_tv3d", _tv_args(a, grad=a + 64), "overlap"),
            ("ddrr_recon_tv3d", _tv_args(a, vol=a + 2), "4-byte aligned"),
            ("ddrr_recon_tv3d", _tv_args(a, grad=a + 4098), "4-byte aligned"),
            ("ddrr_recon_tv3d", _tv_args(a, ws=a + 8), "16-byte aligned"),
            ("ddrr_recon_tv3d", _tv_args(a, ws_bytes=4), "workspace_bytes"),
            ("ddrr_recon_adam_step", _adam_args(a, p=None), "null param"),
            ("ddrr_recon_adam_step", _adam_args(a, g=None), "null grad"),
            ("ddrr_recon_adam_step", _adam_args(a, m=None), "null exp_avg"),
            ("ddrr_recon_adam_step", _adam_args(a, v=None), "null exp_avg_sq"),
            ("ddrr_recon_adam_step", _adam_args(a, step=None), "null step"),
            ("ddrr_recon_adam_step", _adam_args(a, n=-1), "n must be"),
            ("ddrr_recon_adam_step", _adam_args(a, n=2**40 + 1), "n must be"),
            ("ddrr_recon_adam_step", _adam_args(a, lr=-0.1), "lr"),
            ("ddrr_recon_adam_step", _adam_args(a, lr=nan), "lr"),
            ("ddrr_recon_adam_step", _adam_args(a, b1=1.0), "beta1"),
            ("ddrr_recon_adam_step", _adam_args(a, b2=-0.1), "beta1, beta2"),
            ("ddrr_recon_adam_step", _adam_args(a, eps=-1.0), "eps"),
            ("ddrr_recon_adam_step", _adam_args(a, lower=1.0, upper=0.0), "lower"),
            ("ddrr_recon_adam_step", _adam_args(a, lower=nan), "lower"),
            ("ddrr_recon_adam_step", _adam_args(a, p=a + 2), "4-byte aligned")):
        with pytest.raises(RuntimeError, match=what):
            recon.call(name, *args)
    # empty inputs are valid no-ops (nothing is launched)
    assert recon.cdll.ddrr_recon_tv3d(*_tv_args(a, dims=(0, 4, 4))) == 0
    assert recon.cdll.ddrr_recon_tv3d(*_tv_args(a, dims=(4, 4, 0), grad=a + 4096)) == 0
    assert recon.cdll.ddrr_recon_adam_step(*_adam_args(a, n=0)) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_recon_lib", None)
    monkeypatch.setattr(_lib, "RECON_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_recon_lib()
