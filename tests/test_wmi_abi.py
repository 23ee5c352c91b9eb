"""The C ABI of the weighted MutualInformation library: include/diffdrr_wmi_hip.h <-> ctypes signatures <->
libdiffdrr_wmi_hip.so.  No compute is issued here (no GPU needed)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT
from diffdrr_amd import _lib

HEADER = os.path.join(ROOT, "include", "diffdrr_wmi_hip.h")
ENTRIES = {"ddrr_wmi_abi_version", "ddrr_wmi_last_error", "ddrr_wmi_workspace_bytes", "ddrr_wmi_state_floats",
           "ddrr_wmi_forward", "ddrr_wmi_backward"}
KERNELS = ("wmi_joint_kernel", "wmi_reduce_kernel", "wmi_epilogue_kernel") + tuple(
    "wmi_grad_kernelILi%dE" % ns for ns in (1, 4, 16, 32, 64, 128))
OTHERS = ("EXPORTS", "MI_EXPORTS", "RECON_EXPORTS", "FBP_EXPORTS", "LM_EXPORTS", "WARP_EXPORTS", "BSPLINE_EXPORTS",
          "POLYRIGID_EXPORTS", "JACOBIAN_EXPORTS", "PROX_EXPORTS", "WNCC_EXPORTS", "WLM_EXPORTS", "MVLM_EXPORTS",
          "WMVLM_EXPORTS")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|long|const char \*)\s*(ddrr_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return decls


@pytest.fixture(scope="module")
def wmi():
    import __graft_entry__ as entry

    entry.build_wmi_hip()
    return _lib.wmi_library(_lib.WMI_LIB_PATH)


def test_header_matches_ctypes_signatures():
    decls = _declared()
    assert set(decls) == set(_lib.WMI_EXPORTS) == ENTRIES
    for name, argtypes in _lib._WMI_SIGNATURES.items():
        assert decls[name] == len(argtypes), name
    for other in OTHERS:  # no entry shared with any other library
        assert not set(decls) & set(getattr(_lib, other)), other
        assert not any(n.startswith("ddrr_wmi") for n in getattr(_lib, other)), other
    P, I, F, L = _lib._P, _lib._I, _lib._F, _lib._L
    sig = _lib._WMI_SIGNATURES
    assert sig["ddrr_wmi_workspace_bytes"] == [I, I, I, I] and sig["ddrr_wmi_state_floats"] == [I]
    assert sig["ddrr_wmi_forward"] == [P, L, P, L, P, L, I, I, I, P, I, P, F, I, P, L, P, P, P, P]
    assert sig["ddrr_wmi_backward"] == [P, L, P, L, P, L, I, I, I, P, I, P, P, I, P, I, P, P]
    assert _lib._WMI_RESTYPES == {"ddrr_wmi_workspace_bytes": L, "ddrr_wmi_state_floats": L}
    # the unweighted entries with the weight and its stride after the images (and weight_sum before the stream)
    mi = _lib._MI_SIGNATURES
    assert sig["ddrr_wmi_forward"] == mi["ddrr_mi_forward"][:4] + [P, L] + mi["ddrr_mi_forward"][4:-1] + [P, P]
    assert sig["ddrr_wmi_backward"] == mi["ddrr_mi_backward"][:4] + [P, L] + mi["ddrr_mi_backward"][4:]


def test_header_constants_match_and_the_unweighted_header_is_untouched():
    const = dict(re.findall(r"#define (DDRR_WMI_\w+) (\d+)", open(HEADER).read()))
    assert int(const["DDRR_WMI_ABI_VERSION"]) == _lib.WMI_ABI_VERSION == 1
    assert int(const["DDRR_WMI_MAX_BINS"]) == _lib.WMI_MAX_BINS == _lib.MI_MAX_BINS == 256
    assert _lib.MI_ABI_VERSION == 1 and len(_lib.MI_EXPORTS) == 6


def test_library_builds_loads_and_exports_exactly_the_header(wmi):
    assert wmi.cdll.ddrr_wmi_abi_version() == _lib.WMI_ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.WMI_LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    every = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert every == set(_declared()), every ^ set(_declared())


def test_build_calls_the_library_build_and_the_unweighted_library_does_not_depend_on_it():
    import inspect

    import __graft_entry__ as entry

    assert "build_wmi_hip()" in inspect.getsource(entry.build)
    assert entry.WMI_LIB == _lib.WMI_LIB_PATH
    assert "wmi.hip" not in entry.HIP_SOURCES
    assert "wmi" not in inspect.getsource(entry.build_mi_hip)


def test_library_contains_gfx950_code_object(wmi):
    blob = open(_lib.WMI_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert all(k.encode() in blob for k in KERNELS)
    assert b"mi_joint_kernel" in blob and b"15mi_joint_kernel" not in blob  # (its own kernels, not mi.hip's names)


def test_kernels_use_no_scratch_memory_and_the_joint_kernel_keeps_two_workgroups_a_cu(wmi):
    """Read the kernel descriptors of the built code object (as tests/test_wncc_abi.py does): no private segment in
    any kernel; the joint kernel within 256 registers (two waves a SIMD, its launch bound) and within 64 KiB of LDS
    (two workgroups share a CU's 160 KiB)."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(_lib.WMI_LIB_PATH, "rb").read()
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
            path = os.path.join(ROOT, "tests", "emu", "_co_wmi.elf")
            with open(path, "wb") as f:
                f.write(data[off + o:off + o + size])
            try:
                notes = subprocess.run([readelf, "--notes", path], capture_output=True, text=True).stdout
            finally:
                os.remove(path)
            name = None
            for line in notes.splitlines():  # kernel-level keys come in alphabetical order
                m2 = re.match(r"\s+\.(group_segment_fixed_size|name|private_segment_fixed_size|vgpr_count):\s+(\S+)", line)
                if not m2:
                    continue
                key, val = m2.groups()
                if key == "group_segment_fixed_size":
                    lds = int(val)
                elif key == "name" and val.startswith("_Z"):
                    name = val
                elif key == "private_segment_fixed_size" and name is not None:
                    kernels[name] = [int(val), None, lds]
                elif key == "vgpr_count" and name in kernels:
                    kernels[name][1] = int(val)
                    name = None
    for k in KERNELS:
        assert sum(k in name for name in kernels) == 1, (k, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name, (scratch, vgpr, lds) in kernels.items():
        assert scratch == 0, (name, scratch)
        assert vgpr is not None and vgpr <= 256, (name, vgpr)
        if "wmi_joint_kernel" in name:
            assert lds <= 64 * 1024, (name, lds)


# ------------------------------------------------------------------------------------------------ argument rules
_FWD = ("x1", "x2", "w", "bins", "sigma", "workspace", "out")
_BWD = ("x1", "x2", "w", "bins", "sigma", "state", "g_out", "grad")


def _fwd(a, null=None, B=1, H=4, W=4, K=8, s1=16, s2=16, sw=16, eps=1e-10, ws_bytes=1 << 20, ws_off=1024):
    p = {n: a + 64 * i for i, n in enumerate(_FWD)}
    p["workspace"] = a + ws_off
    if null:
        p[null] = None
    return (p["x1"], s1, p["x2"], s2, p["w"], sw, B, H, W, p["bins"], K, p["sigma"], eps, 1, p["workspace"], ws_bytes,
            p["out"], None, None, None)


def _bwd(a, null=None, B=1, H=4, W=4, K=8, s1=16, s2=16, sw=16, which=1, gs=1):
    p = {n: a + 64 * i for i, n in enumerate(_BWD)}
    if null:
        p[null] = None
    return (p["x1"], s1, p["x2"], s2, p["w"], sw, B, H, W, p["bins"], K, p["sigma"], p["state"], which, p["g_out"], gs,
            p["grad"], None)


_ARGS = {"ddrr_wmi_forward": _fwd, "ddrr_wmi_backward": _bwd}


def test_every_entry_rejects_null_pointers_and_negative_sizes_before_any_launch(wmi):
    buf = (ctypes.c_char * 4096)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    status_entries = [n for n in _lib._WMI_SIGNATURES if n not in _lib._WMI_RESTYPES]
    assert status_entries == list(_ARGS)
    for name in status_entries:
        argtypes = _lib._WMI_SIGNATURES[name]
        for pointers, ints, expect in ((None, 0, "null"), (addr, -1, None)):
            args = [pointers if t is _lib._P else (ints if t in (_lib._I, _lib._L) else 0.0) for t in argtypes]
            args[-1] = None  # the stream
            rc = getattr(wmi.cdll, name)(*args)
            msg = wmi.cdll.ddrr_wmi_last_error().decode(errors="replace")
            assert rc == -1 and msg, (name, rc, msg)
            assert "hip" not in msg.lower() and "device" not in msg.lower(), (name, msg)
            if expect:
                assert expect in msg, (name, msg)
        with pytest.raises(RuntimeError, match=name):
            wmi.call(name, *[None if t is _lib._P else (0 if t in (_lib._I, _lib._L) else 0.0) for t in argtypes])
    # the size queries: -1 for invalid sizes; the unweighted library's workspace plus 8 B (chunks + 1) bytes
    assert wmi.query("ddrr_wmi_workspace_bytes", -1, 4, 4, 8) == -1
    assert wmi.query("ddrr_wmi_workspace_bytes", 1, 0, 4, 8) == -1
    assert wmi.query("ddrr_wmi_workspace_bytes", 1, 4, 4, 257) == -1
    assert wmi.query("ddrr_wmi_workspace_bytes", 0, 4, 4, 8) == 0
    assert wmi.query("ddrr_wmi_workspace_bytes", 8, 256, 256, 256) < 64 * 2**20
    assert wmi.query("ddrr_wmi_state_floats", 0) == -1
    assert wmi.query("ddrr_wmi_state_floats", 256) == 256 * 256 + 2 * 256
    import __graft_entry__ as entry
    from mi_cases import geometry

    entry.build_mi_hip()
    mi = _lib.mi_library(_lib.MI_LIB_PATH)
    for B, H, W, K in ((1, 4, 4, 8), (3, 19, 23, 65), (8, 256, 256, 256), (70, 32, 32, 256), (24, 32, 32, 256)):
        chunks = geometry(B, H * W, K)["chunks"]
        assert (wmi.query("ddrr_wmi_workspace_bytes", B, H, W, K)
                == mi.query("ddrr_mi_workspace_bytes", B, H, W, K) + 8 * B * (chunks + 1)), (B, H, W, K)
        assert wmi.query("ddrr_wmi_state_floats", K) == mi.query("ddrr_mi_state_floats", K)


def test_argument_rules(wmi):
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 15) & ~15
    cases = [("ddrr_wmi_forward", _fwd(a, null=n), f"null {n} pointer") for n in _FWD]
    cases += [("ddrr_wmi_backward", _bwd(a, null=n), f"null {n} pointer") for n in _BWD]
    for name, make in _ARGS.items():
        cases += [(name, make(a, K=0), "num_bins"), (name, make(a, K=257), "num_bins"), (name, make(a, B=-1), "B must"),
                  (name, make(a, B=65536), "65535"), (name, make(a, H=0), "H and W"), (name, make(a, W=-2), "H and W"),
                  (name, make(a, s1=5), "x1_stride"), (name, make(a, s2=-16), "x2_stride"),
                  (name, make(a, sw=5), "w_stride"), (name, make(a, sw=-16), "w_stride")]
    cases += [("ddrr_wmi_forward", _fwd(a, eps=-1.0), "epsilon"), ("ddrr_wmi_forward", _fwd(a, eps=float("nan")), "epsilon"),
              ("ddrr_wmi_forward", _fwd(a, ws_bytes=16), "workspace_bytes"),
              ("ddrr_wmi_forward", _fwd(a, ws_off=1028), "16-byte aligned"),
              ("ddrr_wmi_backward", _bwd(a, which=2), "which"), ("ddrr_wmi_backward", _bwd(a, gs=3), "g_stride")]
    for name, args, what in cases:
        with pytest.raises(RuntimeError, match=what):
            wmi.call(name, *args)
    # an empty batch is a valid no-op (nothing is launched); a shared weight (stride 0) is a valid argument
    for name, make in _ARGS.items():
        assert getattr(wmi.cdll, name)(*make(a, B=0)) == 0, name
        assert getattr(wmi.cdll, name)(*make(a, B=0, sw=0, s1=0)) == 0, name


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_wmi_lib", None)
    monkeypatch.setattr(_lib, "WMI_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="have not been built"):
        _lib.get_wmi_lib()
    from diffdrr_amd import ops

    with pytest.raises(RuntimeError, match="have not been built"):
        ops._query_wmi("ddrr_wmi_state_floats", 8)
