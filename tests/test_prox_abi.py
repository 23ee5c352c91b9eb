"""The C ABI of the TV proximal operator library: include/diffdrr_prox_hip.h <-> ctypes signatures <->
libdiffdrr_prox_hip.so, and the argument errors through ``ops.prox_tv3d``.  No compute is issued on a device here
(no GPU needed)."""
import ctypes
import math
import os
import re
import struct
import subprocess

import pytest
import torch

import prox_cases
from conftest import ROOT
from diffdrr_amd import _lib, ops

HEADER = os.path.join(ROOT, "include", "diffdrr_prox_hip.h")
ENTRIES = {"ddrr_prox_abi_version", "ddrr_prox_last_error", "ddrr_prox_workspace_bytes", "ddrr_prox_tv3d"}
# (the primal kernel with and without the epilogue, the dual kernel once per mode)
KERNELS = {"prox_primal_kernel": 2, "prox_dual_kernel": 2}


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def prox():
    import __graft_entry__ as entry

    entry.build_prox_hip()
    return _lib.prox_library(_lib.PROX_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.PROX_EXPORTS) == ENTRIES
    for name, argtypes in _lib._PROX_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    for other in (_lib.EXPORTS, _lib.MI_EXPORTS, _lib.RECON_EXPORTS, _lib.FBP_EXPORTS, _lib.LM_EXPORTS,
                  _lib.WARP_EXPORTS, _lib.BSPLINE_EXPORTS, _lib.POLYRIGID_EXPORTS, _lib.JACOBIAN_EXPORTS):
        assert not set(decls) & set(other)
    P, I, L, F = _lib._P, _lib._I, _lib._L, _lib._F
    assert _lib._PROX_SIGNATURES["ddrr_prox_workspace_bytes"] == [I] * 4
    assert _lib._PROX_SIGNATURES["ddrr_prox_tv3d"] == [P, I, I, I, F, F, F, I, F, I, F, F, P, P, L, P, P, F, P, P]
    assert _lib._PROX_RESTYPES == {"ddrr_prox_workspace_bytes": L}


def test_header_constants_match():
    const = dict(re.findall(r"#define (DDRR_PROX_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_PROX_ABI_VERSION"]) == _lib.PROX_ABI_VERSION == 1
    assert (int(const["DDRR_PROX_TV_ISOTROPIC"]), int(const["DDRR_PROX_TV_ANISOTROPIC"])) == \
        (_lib.PROX_TV_ISOTROPIC, _lib.PROX_TV_ANISOTROPIC) == (_lib.RECON_TV_ISOTROPIC, _lib.RECON_TV_ANISOTROPIC)
    assert int(const["DDRR_PROX_MAX_DIM"]) == _lib.PROX_MAX_DIM == _lib.RECON_MAX_DIM == 65535


def test_the_other_headers_and_their_versions_are_untouched():
    assert (_lib.ABI_VERSION, _lib.MI_ABI_VERSION, _lib.RECON_ABI_VERSION, _lib.FBP_ABI_VERSION, _lib.LM_ABI_VERSION,
            _lib.WARP_ABI_VERSION, _lib.BSPLINE_ABI_VERSION, _lib.POLYRIGID_ABI_VERSION, _lib.JACOBIAN_ABI_VERSION) == \
        (33, 1, 1, 1, 1, 1, 1, 1, 1)
    assert set(_lib.RECON_EXPORTS) == {"ddrr_recon_abi_version", "ddrr_recon_last_error",
                                       "ddrr_recon_tv_workspace_bytes", "ddrr_recon_tv3d", "ddrr_recon_adam_step"}


def test_library_builds_loads_and_exports_exactly_the_header(prox):
    assert prox.cdll.ddrr_prox_abi_version() == _lib.PROX_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.PROX_LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_emulation_exports_the_header():
    assert prox_cases.emu_library().cdll.ddrr_prox_abi_version() == _lib.PROX_ABI_VERSION


def test_build_calls_the_library_build():
    import inspect

    import __graft_entry__ as entry

    assert "build_prox_hip()" in inspect.getsource(entry.build)
    assert entry.PROX_LIB == _lib.PROX_LIB_PATH
    assert "prox_core.h" not in entry.HIP_HEADERS  # (the main library does not rebuild for it)
    assert "prox_library(PROX_LIB)" in inspect.getsource(entry.build)


def test_library_contains_gfx950_code_object(prox):
    blob = open(_lib.PROX_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)


def test_kernels_use_no_scratch_memory(prox):
    """Read the kernel descriptors of the built code object (as tests/test_jacobian_abi.py does): no private
    segment in any kernel; at most 128 registers (four waves per SIMD) in the primal kernels and 168 (three) in
    the dual ones, which hold p, r and the next plane's x at once; the counts are printed."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.PROX_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_prox.elf")
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
        assert vgpr is not None and vgpr <= (168 if "prox_dual_kernel" in name else 128), (name, vgpr)


N = 2 * 3 * 4 * 4  # bytes of a (2, 3, 4) volume


def _args(a, null=None, dims=(2, 3, 4), spacing=(1.0, 1.0, 1.0), mode=0, lam=0.1, iterations=2, lower=-math.inf,
          upper=math.inf, scratch_bytes=3 * N, beta=0.5, epilogue=True, **at):
    """Valid host-side arguments of ddrr_prox_tv3d (nothing is launched for the cases that use them); `at`
    moves a pointer to a + offset."""
    ptr = {"b": a, "dual": a + 1024, "scratch": a + 2048, "x_out": a + 3072, "x_prev": a + 4096, "y_out": a + 5120}
    if not epilogue:
        ptr["x_prev"] = ptr["y_out"] = None
    for k, off in at.items():
        ptr[k] = a + off
    if null is not None:
        ptr[null] = None
    return (ptr["b"], *dims, *spacing, mode, lam, iterations, lower, upper, ptr["dual"], ptr["scratch"],
            scratch_bytes, ptr["x_out"], ptr["x_prev"], beta, ptr["y_out"], None)


RULES = [
    (dict(null="b"), "null b pointer"),
    (dict(null="dual"), "null dual pointer"),
    (dict(null="x_out"), "null x_out pointer"),
    (dict(null="scratch"), "null scratch pointer"),
    (dict(null="x_prev"), "both be given or both be null"),
    (dict(null="y_out"), "both be given or both be null"),
    (dict(dims=(2, -3, 4)), ">= 0"),
    (dict(dims=(65536, 1, 1)), "<= 65535"),
    (dict(dims=(65535, 65535, 5)), r"<= 2\^34"),
    (dict(spacing=(1.0, 0.0, 1.0)), "sx, sy, sz must be > 0 and finite"),
    (dict(spacing=(1.0, 1.0, math.inf)), "sx, sy, sz must be > 0 and finite"),
    (dict(spacing=(math.nan, 1.0, 1.0)), "sx, sy, sz must be > 0 and finite"),
    (dict(mode=2), "mode must be"),
    (dict(lam=-0.1), "lambda must be >= 0 and finite"),
    (dict(lam=math.inf), "lambda must be >= 0 and finite"),
    (dict(lam=math.nan), "lambda must be >= 0 and finite"),
    (dict(iterations=-1), "iterations must be >= 0"),
    (dict(lower=1.0, upper=0.5), "lower must be <= upper"),
    (dict(lower=math.nan), "lower must be <= upper"),
    (dict(beta=math.inf), "beta must be finite"),
    (dict(b=2), "4-byte aligned"),
    (dict(dual=1025), "4-byte aligned"),
    (dict(x_out=3073), "4-byte aligned"),
    (dict(scratch_bytes=3 * N - 1), "scratch_bytes is smaller"),
    (dict(x_out=N - 4), "x_out must not overlap b"),
    (dict(y_out=4), "y_out must not overlap b"),
    (dict(dual=N - 4), "dual must not overlap b"),
    (dict(scratch=8), "scratch must not overlap b"),
    (dict(x_out=4096), "x_out must not overlap x_prev, dual or scratch"),
    (dict(x_out=1024 + 3 * N - 4), "x_out must not overlap x_prev, dual or scratch"),
    (dict(y_out=3072 + N - 4), "y_out must not overlap x_out, dual or scratch"),
    (dict(scratch=1024 + 4), "scratch must not overlap dual"),
    (dict(x_prev=1024 + 8), "x_prev must not overlap dual or scratch"),
    (dict(x_prev=2048 + 3 * N - 4), "x_prev must not overlap dual or scratch"),
]


@pytest.mark.parametrize("build", ["product", "emulation"])
def test_argument_rules(prox, build):
    lib = prox if build == "product" else prox_cases.emu_library()
    buf = (ctypes.c_char * 16384)()
    a = (ctypes.addressof(buf) + 15) & ~15
    for kw, what in RULES:
        rc = lib.cdll.ddrr_prox_tv3d(*_args(a, **kw))
        msg = lib.cdll.ddrr_prox_last_error().decode(errors="replace")
        assert rc == -1 and re.search(what, msg), (kw, rc, msg)
        assert "hip" not in msg.lower(), msg
        with pytest.raises(RuntimeError, match="ddrr_prox_tv3d failed"):
            lib.call("ddrr_prox_tv3d", *_args(a, **kw))
    # an empty volume is a no-op, whatever the pointers hold; no scratch is needed without iterations or lambda
    assert lib.cdll.ddrr_prox_tv3d(*_args(a, dims=(0, 3, 4))) == 0
    assert lib.cdll.ddrr_prox_tv3d(*_args(a, dims=(2, 0, 4), null="scratch", epilogue=False)) == 0
    assert lib.query("ddrr_prox_workspace_bytes", 2, 3, 4, 2) == 3 * N
    assert lib.query("ddrr_prox_workspace_bytes", 2, 3, 4, 0) == 0
    assert lib.query("ddrr_prox_workspace_bytes", 0, 3, 4, 5) == 0
    assert lib.query("ddrr_prox_workspace_bytes", 2048, 2048, 4096, 1) == 3 * 4 * 2 ** 34
    assert lib.query("ddrr_prox_workspace_bytes", -1, 3, 4, 2) == -1
    assert lib.query("ddrr_prox_workspace_bytes", 2, 3, 4, -2) == -1
    assert lib.query("ddrr_prox_workspace_bytes", 65536, 3, 4, 2) == -1


def test_the_emulation_runs_what_the_rules_allow():
    """lambda == 0 and iterations == 0 need no scratch; y_out may be x_prev itself."""
    lib = prox_cases.emu_library()
    b = prox_cases.volume((2, 3, 4), "step")
    dual, x, xp = torch.zeros(3, 2, 3, 4), torch.empty(2, 3, 4), torch.zeros(2, 3, 4)
    inf = math.inf
    for lam, n in ((0.0, 5), (0.3, 0)):
        lib.call("ddrr_prox_tv3d", b.data_ptr(), 2, 3, 4, 1.0, 1.0, 1.0, 0, lam, n, 0.5, inf, dual.data_ptr(), None, 0,
                 x.data_ptr(), None, 0.0, None, None)
        assert torch.equal(x, b.clamp(min=0.5))
    lib.call("ddrr_prox_tv3d", b.data_ptr(), 2, 3, 4, 1.0, 1.0, 1.0, 0, 0.0, 0, -inf, inf, dual.data_ptr(), None, 0,
             x.data_ptr(), xp.data_ptr(), 1.0, xp.data_ptr(), None)
    assert torch.equal(x, b) and torch.equal(xp, 2 * b)


def test_ops_raise_each_rule_by_name(monkeypatch):
    """Item 9: what Python can check is a ValueError before the library is reached; what only the library sees
    (overlapping tensors) comes back as its RuntimeError."""
    prox_cases.route_prox_to_emulation(monkeypatch, ops)
    b = prox_cases.volume((2, 3, 4), "step")
    dual = torch.zeros(3, 2, 3, 4)
    good = dict(lam=0.1, spacing=(1.0, 1.0, 1.0), mode="isotropic", iterations=2, dual=dual)
    x, y = ops.prox_tv3d(b, **good)
    assert y is None and x.shape == b.shape
    for kw, what in ((dict(lam=-1.0), "lam must be >= 0"), (dict(lam=math.inf), "lam must be >= 0"),
                     (dict(lam=math.nan), "lam must be >= 0"), (dict(spacing=(1.0, -1.0, 1.0)), "spacing"),
                     (dict(spacing=(1.0, 1.0)), "spacing"), (dict(mode="huber"), "mode must be"),
                     (dict(iterations=-1), "iterations"), (dict(iterations=1.5), "iterations"),
                     (dict(lower=1.0, upper=0.0), "lower 1.0 must be <= upper 0.0"),
                     (dict(lower=math.nan), "must be <="), (dict(dual=None), "dual is required"),
                     (dict(dual=torch.zeros(3, 2, 3, 5)), "dual must be"),
                     (dict(dual=torch.zeros(3, 2, 3, 4, dtype=torch.float64)), "dual must be"),
                     (dict(dual=torch.zeros(3, 2, 3, 8)[..., ::2]), "dual must be"),
                     (dict(x_prev=torch.zeros(2, 3, 5)), "x_prev"),
                     (dict(x_prev=torch.zeros(2, 3, 4), beta=math.inf), "beta must be finite")):
        with pytest.raises(ValueError, match=what):
            ops.prox_tv3d(b, **{**good, **kw})
    for bad, what in ((b.double(), "float32"), (b.transpose(0, 1), "contiguous"), (b[0], r"\(Dx, Dy, Dz\)")):
        with pytest.raises(ValueError, match=what):
            ops.prox_tv3d(bad, **good)
    shared = torch.zeros(4 * b.numel())
    shared[:b.numel()] = b.flatten()
    with pytest.raises(RuntimeError, match="dual must not overlap b"):
        ops.prox_tv3d(shared[:24].view(2, 3, 4), **{**good, "dual": shared[12:84].view(3, 2, 3, 4)})
    with pytest.raises(RuntimeError, match="x_prev must not overlap dual"):
        ops.prox_tv3d(b, **{**good, "x_prev": dual[0]})


def test_cpu_tensors_are_rejected_without_the_emulation():
    with pytest.raises(ValueError, match="GPU"):
        ops.prox_tv3d(torch.zeros(2, 3, 4), 0.1, dual=torch.zeros(3, 2, 3, 4))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_prox_lib", None)
    monkeypatch.setattr(_lib, "PROX_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_prox_lib()
    with pytest.raises(RuntimeError, match="have not been built"):
        ops._query_prox("ddrr_prox_workspace_bytes", 2, 2, 2, 1)
