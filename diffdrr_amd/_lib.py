"""ctypes binding of ``libdiffdrr_hip.so`` (C ABI: ``include/diffdrr_hip.h``).

The library is built in-tree by ``__graft_entry__.build()`` (``hipcc
--offload-arch=gfx950``) and loaded *after* torch so that it binds to the HIP
runtime torch already has in the process (same ``libamdhip64.so.7`` soname):
kernels can then be launched on torch's current stream with torch's device
pointers.  There is deliberately no CPU or pure-PyTorch fallback: if the
library is missing, rendering raises.

The headers are the only place the binding's types are written down: every entry's ctypes argument
and result types, and the ``DDRR_*`` constants Python uses, are read from them when this module is
imported (:func:`parse_header`).  A declaration the parser cannot map exactly is an error, never a
guess.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_void_p
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_hip.so")
# The ABI versions ops.py is written against: the header's DDRR_*ABI_VERSION and the loaded library's
# own must both be these (checked on import and on load).
ABI_VERSION = 33
MI_ABI_VERSION = 1
RECON_ABI_VERSION = 1
FBP_ABI_VERSION = 1
LM_ABI_VERSION = 1
WARP_ABI_VERSION = 1
BSPLINE_ABI_VERSION = 1
POLYRIGID_ABI_VERSION = 1
JACOBIAN_ABI_VERSION = 1
PROX_ABI_VERSION = 1
WNCC_ABI_VERSION = 1
WLM_ABI_VERSION = 1
MVLM_ABI_VERSION = 1
WMVLM_ABI_VERSION = 1
WMI_ABI_VERSION = 1

_P, _I, _F, _L, _D = c_void_p, c_int, c_float, c_long, c_double
_ARGTYPES = {"int": c_int, "long": c_long, "float": c_float, "double": c_double}
_RESTYPES_OF = {"int": c_int, "long": c_long, "const char *": c_char_p}
_DECLARATION = re.compile(r"(.*?)\b(ddrr_\w+)\s*\((.*)\)", re.S)
_POINTER = re.compile(r"[\w\s]+\*[\s*]*\w+")   # T *name, const T *name, T **name
_SCALAR = re.compile(r"(\w+)\s+\w+")            # T name


def parse_header(text: str):
    """The entries of a C header -- every declaration ``int|long|const char * ddrr_...(...);`` -- and its
    integer ``#define DDRR_*`` constants.  Any pointer is ``c_void_p``; ``int``, ``long``, ``float`` and
    ``double`` map to their ctypes; a return type other than ``int``, ``long`` or ``const char *``, any
    other parameter type (``unsigned``, ``size_t``, ``bool``, a function pointer) or a declaration that
    does not read as one raises ValueError naming the entry.
    -> (name -> argtypes, name -> restype, DDRR_NAME -> int), entries in the header's order"""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    code = re.sub(r"//[^\n]*", "", code)
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DDRR_\w+)[ \t]+(\d+)[ \t]*$",
                                                code, re.M)}
    code = re.sub(r"^[ \t]*#[^\n]*", "", code, flags=re.M)
    signatures, restypes = {}, {}
    for stmt in re.split(r"[;{}]", code):
        if not re.search(r"\bddrr_\w+\s*\(", stmt):
            continue
        m = _DECLARATION.fullmatch(" ".join(stmt.split()))
        name = m.group(2) if m else re.search(r"\bddrr_\w+", stmt).group(0)
        ret = re.sub(r"\s*\*\s*", " *", m.group(1)).strip() if m else None
        if ret not in _RESTYPES_OF:
            raise ValueError(f"{name}: cannot bind the declaration {' '.join(stmt.split())!r} "
                             "(return type int, long or const char * expected)")
        params = m.group(3).strip()
        argtypes = []
        for param in ([] if params == "void" else params.split(",")):
            param = param.strip()
            scalar = _SCALAR.fullmatch(param)
            if _POINTER.fullmatch(param):
                argtypes.append(c_void_p)
            elif scalar and scalar.group(1) in _ARGTYPES:
                argtypes.append(_ARGTYPES[scalar.group(1)])
            else:
                raise ValueError(f"{name}: cannot bind the parameter {param!r} (a pointer, int, long, float "
                                 "or double expected)")
        if name in signatures:
            raise ValueError(f"{name}: declared twice")
        signatures[name], restypes[name] = argtypes, _RESTYPES_OF[ret]
    return signatures, restypes, defines


class Header(NamedTuple):
    """The C ABI one header declares, as the binding uses it."""
    path: str
    prefix: str         # of the entries every such library has: <prefix>_abi_version, <prefix>_last_error
    version: int        # the ABI version the Python side is written against
    argtypes: dict      # every entry -> ctypes argument types
    restypes: dict      # every entry -> ctypes result type
    defines: dict       # DDRR_* -> int

    @classmethod
    def read(cls, name: str, prefix: str, version: int) -> "Header":
        path = os.path.join(_INCLUDE, name)
        with open(path) as f:
            argtypes, restypes, defines = parse_header(f.read())
        macro = f"{prefix.upper()}_ABI_VERSION"
        if defines.get(macro) != version:
            raise RuntimeError(f"{path}: {macro} is {defines.get(macro)}, the binding is written against {version}")
        return cls(path, prefix, version, argtypes, restypes, defines)

    def tables(self):
        """-> (signatures, restypes, exports): the status- and size-returning entries (all but
        <prefix>_abi_version and <prefix>_last_error) -> argtypes, those of them that return a size
        -> restype, every entry's name"""
        own = (f"{self.prefix}_abi_version", f"{self.prefix}_last_error")
        signatures = {n: a for n, a in self.argtypes.items() if n not in own}
        return signatures, {n: self.restypes[n] for n in signatures if self.restypes[n] is not c_int}, \
            list(self.argtypes)

    def constants(self, *names):
        return [self.defines[f"{self.prefix.upper()}_{n}"] for n in names]


HEADER = Header.read("diffdrr_hip.h", "ddrr", ABI_VERSION)
_SIGNATURES, _RESTYPES, EXPORTS = HEADER.tables()

REDUCE_SUM, REDUCE_MAX = HEADER.constants("REDUCE_SUM", "REDUCE_MAX")
LOOKUP_STEP, LOOKUP_MID_NEAREST, LOOKUP_MID_TRILINEAR = HEADER.constants(
    "LOOKUP_STEP", "LOOKUP_MID_NEAREST", "LOOKUP_MID_TRILINEAR")
SIDDON_AUX, = HEADER.constants("SIDDON_AUX")
AUX_INTERLEAVED, AUX_BLOCKED, AUX_PACKED = HEADER.constants("AUX_INTERLEAVED", "AUX_BLOCKED", "AUX_PACKED")
REC_BLOCK_RAYS, REC_BLOCK_FLOATS = HEADER.constants("REC_BLOCK_RAYS", "REC_BLOCK_FLOATS")  # csrc/record_layout.h
# how a brick is held in LDS (ddrr_siddon_forward_bricks); BRICKS_CLEARED is a bit of ranges_valid
BRICKS_F32, BRICKS_Q16, BRICKS_Q16_PACKED, BRICKS_CLEARED = HEADER.constants(
    "BRICKS_F32", "BRICKS_Q16", "BRICKS_Q16_PACKED", "BRICKS_CLEARED")
BRICKS_Q16_Y, BRICKS_Q16_PACKED_Y = HEADER.constants("BRICKS_Q16_Y", "BRICKS_Q16_PACKED_Y")  # 32 x 64 x 32 bricks
PACKED_AUX_PLANES, TRI_AUX_PLANES = HEADER.constants("PACKED_AUX_PLANES", "TRI_AUX_PLANES")


class DdrrLibrary:
    """A loaded implementation of the C ABI of ``header`` (the HIP product library; the tests also bind
    their host emulation build through this class; :func:`mi_library` binds the MutualInformation
    library, include/diffdrr_mi_hip.h).  Checks that every entry of the header is exported and that the
    library's ABI version is the binding's."""

    def __init__(self, path: str, header: Header = HEADER):
        self.path = path
        self.cdll = ctypes.CDLL(path)
        for name in header.argtypes:
            if not hasattr(self.cdll, name):
                raise RuntimeError(f"{path} does not export {name}")
            fn = getattr(self.cdll, name)
            fn.argtypes, fn.restype = header.argtypes[name], header.restypes[name]
        got = getattr(self.cdll, f"{header.prefix}_abi_version")()
        if got != header.version:
            raise RuntimeError(f"{path}: ABI version {got}, expected {header.version}")
        self._last_error = getattr(self.cdll, f"{header.prefix}_last_error")

    def query(self, name: str, *args):
        """An entry that returns a value (``_RESTYPES``), not a status."""
        return getattr(self.cdll, name)(*args)

    def call(self, name: str, *args):
        rc = getattr(self.cdll, name)(*args)
        if rc != 0:
            msg = self._last_error().decode(errors="replace")
            raise RuntimeError(f"{name} failed (code {rc}): {msg}")


_lib: DdrrLibrary | None = None


def get_lib() -> DdrrLibrary:
    """The HIP library, loaded on first use.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the MI355X renderers have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); "
                "diffdrr_amd has no CPU fallback."
            )
        _lib = DdrrLibrary(LIB_PATH)
    return _lib


# ----------------------------------------------------------------- libdiffdrr_mi_hip.so
# MutualInformation (C ABI: include/diffdrr_mi_hip.h): a library of its own, with its own version
MI_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_mi_hip.so")
MI_HEADER = Header.read("diffdrr_mi_hip.h", "ddrr_mi", MI_ABI_VERSION)
_MI_SIGNATURES, _MI_RESTYPES, MI_EXPORTS = MI_HEADER.tables()
MI_MAX_BINS, = MI_HEADER.constants("MAX_BINS")


def mi_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_mi_hip.h."""
    return DdrrLibrary(path, MI_HEADER)


_mi_lib: DdrrLibrary | None = None


def get_mi_lib() -> DdrrLibrary:
    """The MutualInformation library, loaded on first use.  Raises if it has not been built."""
    global _mi_lib
    if _mi_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(MI_LIB_PATH):
            raise RuntimeError(
                f"{MI_LIB_PATH} is missing: the MutualInformation kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _mi_lib = mi_library(MI_LIB_PATH)
    return _mi_lib


# ----------------------------------------------------------------- libdiffdrr_recon_hip.so
# Reconstruction: total variation and the volume's Adam step (C ABI: include/diffdrr_recon_hip.h)
RECON_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_recon_hip.so")
RECON_HEADER = Header.read("diffdrr_recon_hip.h", "ddrr_recon", RECON_ABI_VERSION)
_RECON_SIGNATURES, _RECON_RESTYPES, RECON_EXPORTS = RECON_HEADER.tables()
RECON_TV_ISOTROPIC, RECON_TV_ANISOTROPIC, RECON_MAX_DIM = RECON_HEADER.constants(
    "TV_ISOTROPIC", "TV_ANISOTROPIC", "MAX_DIM")


def recon_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_recon_hip.h."""
    return DdrrLibrary(path, RECON_HEADER)


_recon_lib: DdrrLibrary | None = None


def get_recon_lib() -> DdrrLibrary:
    """The reconstruction library, loaded on first use.  Raises if it has not been built."""
    global _recon_lib
    if _recon_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(RECON_LIB_PATH):
            raise RuntimeError(
                f"{RECON_LIB_PATH} is missing: the reconstruction kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _recon_lib = recon_library(RECON_LIB_PATH)
    return _recon_lib


# ----------------------------------------------------------------- libdiffdrr_fbp_hip.so
# FDK initialisation: projection filter and voxel-driven backprojection (C ABI: include/diffdrr_fbp_hip.h)
FBP_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_fbp_hip.so")
FBP_HEADER = Header.read("diffdrr_fbp_hip.h", "ddrr_fbp", FBP_ABI_VERSION)
_FBP_SIGNATURES, _FBP_RESTYPES, FBP_EXPORTS = FBP_HEADER.tables()
FBP_MAX_IMAGE_DIM, FBP_MAX_VIEWS, FBP_MAX_DIM, FBP_VIEW_FLOATS = FBP_HEADER.constants(
    "MAX_IMAGE_DIM", "MAX_VIEWS", "MAX_DIM", "VIEW_FLOATS")


def fbp_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_fbp_hip.h."""
    return DdrrLibrary(path, FBP_HEADER)


_fbp_lib: DdrrLibrary | None = None


def get_fbp_lib() -> DdrrLibrary:
    """The FDK library, loaded on first use.  Raises if it has not been built."""
    global _fbp_lib
    if _fbp_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(FBP_LIB_PATH):
            raise RuntimeError(
                f"{FBP_LIB_PATH} is missing: the FDK kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _fbp_lib = fbp_library(FBP_LIB_PATH)
    return _fbp_lib


# ----------------------------------------------------------------- libdiffdrr_lm_hip.so
# Levenberg-Marquardt registration: normal-equations sums and the step (C ABI: include/diffdrr_lm_hip.h)
LM_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_lm_hip.so")
LM_HEADER = Header.read("diffdrr_lm_hip.h", "ddrr_lm", LM_ABI_VERSION)
_LM_SIGNATURES, _LM_RESTYPES, LM_EXPORTS = LM_HEADER.tables()
LM_SUMS, LM_GROUP_RAYS, LM_STATE_DOUBLES, LM_MAX_POSES = LM_HEADER.constants(
    "SUMS", "GROUP_RAYS", "STATE_DOUBLES", "MAX_POSES")


def lm_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_lm_hip.h."""
    return DdrrLibrary(path, LM_HEADER)


_lm_lib: DdrrLibrary | None = None


def get_lm_lib() -> DdrrLibrary:
    """The Levenberg-Marquardt library, loaded on first use.  Raises if it has not been built."""
    global _lm_lib
    if _lm_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(LM_LIB_PATH):
            raise RuntimeError(
                f"{LM_LIB_PATH} is missing: the Levenberg-Marquardt kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _lm_lib = lm_library(LM_LIB_PATH)
    return _lm_lib


# ----------------------------------------------------------------- libdiffdrr_warp_hip.so
# Free-form deformation of the volume: the warp and its two adjoints (C ABI: include/diffdrr_warp_hip.h)
WARP_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_warp_hip.so")
WARP_HEADER = Header.read("diffdrr_warp_hip.h", "ddrr_warp", WARP_ABI_VERSION)
_WARP_SIGNATURES, _WARP_RESTYPES, WARP_EXPORTS = WARP_HEADER.tables()
WARP_PADDING_ZEROS, WARP_PADDING_BORDER, WARP_MAX_DIM, WARP_PIECE_VOXELS, WARP_PIECE_FLOATS = WARP_HEADER.constants(
    "PADDING_ZEROS", "PADDING_BORDER", "MAX_DIM", "PIECE_VOXELS", "PIECE_FLOATS")


def warp_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_warp_hip.h."""
    return DdrrLibrary(path, WARP_HEADER)


_warp_lib: DdrrLibrary | None = None


def get_warp_lib() -> DdrrLibrary:
    """The free-form deformation library, loaded on first use.  Raises if it has not been built."""
    global _warp_lib
    if _warp_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(WARP_LIB_PATH):
            raise RuntimeError(
                f"{WARP_LIB_PATH} is missing: the free-form deformation kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _warp_lib = warp_library(WARP_LIB_PATH)
    return _warp_lib


# ----------------------------------------------------------------- libdiffdrr_bspline_hip.so
# Cubic B-spline free-form deformation: the warp and its two adjoints (C ABI: include/diffdrr_bspline_hip.h)
BSPLINE_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_bspline_hip.so")
BSPLINE_HEADER = Header.read("diffdrr_bspline_hip.h", "ddrr_bspline", BSPLINE_ABI_VERSION)
_BSPLINE_SIGNATURES, _BSPLINE_RESTYPES, BSPLINE_EXPORTS = BSPLINE_HEADER.tables()
BSPLINE_PADDING_ZEROS, BSPLINE_PADDING_BORDER, BSPLINE_MAX_DIM, BSPLINE_CHUNK_VOXELS, BSPLINE_ROWS = \
    BSPLINE_HEADER.constants("PADDING_ZEROS", "PADDING_BORDER", "MAX_DIM", "CHUNK_VOXELS", "ROWS")


def bspline_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_bspline_hip.h."""
    return DdrrLibrary(path, BSPLINE_HEADER)


_bspline_lib: DdrrLibrary | None = None


def get_bspline_lib() -> DdrrLibrary:
    """The cubic B-spline deformation library, loaded on first use.  Raises if it has not been built."""
    global _bspline_lib
    if _bspline_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(BSPLINE_LIB_PATH):
            raise RuntimeError(
                f"{BSPLINE_LIB_PATH} is missing: the B-spline deformation kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _bspline_lib = bspline_library(BSPLINE_LIB_PATH)
    return _bspline_lib


# ----------------------------------------------------------------- libdiffdrr_polyrigid_hip.so
# Polyrigid deformation of the volume: the warp and its two adjoints (C ABI: include/diffdrr_polyrigid_hip.h)
POLYRIGID_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_polyrigid_hip.so")
POLYRIGID_HEADER = Header.read("diffdrr_polyrigid_hip.h", "ddrr_polyrigid", POLYRIGID_ABI_VERSION)
_POLYRIGID_SIGNATURES, _POLYRIGID_RESTYPES, POLYRIGID_EXPORTS = POLYRIGID_HEADER.tables()
POLYRIGID_PADDING_ZEROS, POLYRIGID_PADDING_BORDER, POLYRIGID_MAX_DIM, POLYRIGID_PIECE_VOXELS, \
    POLYRIGID_PIECE_FLOATS = POLYRIGID_HEADER.constants(
        "PADDING_ZEROS", "PADDING_BORDER", "MAX_DIM", "PIECE_VOXELS", "PIECE_FLOATS")
# A, B, C of the SE(3) exponential: Taylor series of POLYRIGID_SERIES_TERMS terms in s = |omega|^2 below the seam
POLYRIGID_SERIES_TERMS, _num, _den = POLYRIGID_HEADER.constants(
    "SERIES_TERMS", "SERIES_BELOW_NUM", "SERIES_BELOW_DEN")
POLYRIGID_SERIES_BELOW = _num / _den


def polyrigid_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_polyrigid_hip.h."""
    return DdrrLibrary(path, POLYRIGID_HEADER)


_polyrigid_lib: DdrrLibrary | None = None


def get_polyrigid_lib() -> DdrrLibrary:
    """The polyrigid deformation library, loaded on first use.  Raises if it has not been built."""
    global _polyrigid_lib
    if _polyrigid_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(POLYRIGID_LIB_PATH):
            raise RuntimeError(
                f"{POLYRIGID_LIB_PATH} is missing: the polyrigid deformation kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _polyrigid_lib = polyrigid_library(POLYRIGID_LIB_PATH)
    return _polyrigid_lib


# ----------------------------------------------------------------- libdiffdrr_jacobian_hip.so
# Jacobian determinant of a lattice deformation, folding statistics, volume penalty and their lattice gradient
# (C ABI: include/diffdrr_jacobian_hip.h)
JACOBIAN_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_jacobian_hip.so")
JACOBIAN_HEADER = Header.read("diffdrr_jacobian_hip.h", "ddrr_jacobian", JACOBIAN_ABI_VERSION)
_JACOBIAN_SIGNATURES, _JACOBIAN_RESTYPES, JACOBIAN_EXPORTS = JACOBIAN_HEADER.tables()
JACOBIAN_BASIS_LINEAR, JACOBIAN_BASIS_BSPLINE, JACOBIAN_MAX_DIM, JACOBIAN_PARTIAL_BYTES = \
    JACOBIAN_HEADER.constants("BASIS_LINEAR", "BASIS_BSPLINE", "MAX_DIM", "PARTIAL_BYTES")


def jacobian_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_jacobian_hip.h."""
    return DdrrLibrary(path, JACOBIAN_HEADER)


_jacobian_lib: DdrrLibrary | None = None


def get_jacobian_lib() -> DdrrLibrary:
    """The Jacobian determinant library, loaded on first use.  Raises if it has not been built."""
    global _jacobian_lib
    if _jacobian_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(JACOBIAN_LIB_PATH):
            raise RuntimeError(
                f"{JACOBIAN_LIB_PATH} is missing: the Jacobian determinant kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _jacobian_lib = jacobian_library(JACOBIAN_LIB_PATH)
    return _jacobian_lib


# ----------------------------------------------------------------- libdiffdrr_prox_hip.so
# The proximal operator of the total variation with a box constraint: FISTA reconstruction's inner solver
# (C ABI: include/diffdrr_prox_hip.h)
PROX_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_prox_hip.so")
PROX_HEADER = Header.read("diffdrr_prox_hip.h", "ddrr_prox", PROX_ABI_VERSION)
_PROX_SIGNATURES, _PROX_RESTYPES, PROX_EXPORTS = PROX_HEADER.tables()
PROX_TV_ISOTROPIC, PROX_TV_ANISOTROPIC, PROX_MAX_DIM = PROX_HEADER.constants(
    "TV_ISOTROPIC", "TV_ANISOTROPIC", "MAX_DIM")


def prox_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_prox_hip.h."""
    return DdrrLibrary(path, PROX_HEADER)


_prox_lib: DdrrLibrary | None = None


def get_prox_lib() -> DdrrLibrary:
    """The TV proximal operator library, loaded on first use.  Raises if it has not been built."""
    global _prox_lib
    if _prox_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(PROX_LIB_PATH):
            raise RuntimeError(
                f"{PROX_LIB_PATH} is missing: the TV proximal operator kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _prox_lib = prox_library(PROX_LIB_PATH)
    return _prox_lib


# ----------------------------------------------------------------- libdiffdrr_wncc_hip.so
# Weighted (masked) NCC of image pairs and the registration step's epilogues with a per-pixel weight
# (C ABI: include/diffdrr_wncc_hip.h)
WNCC_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_wncc_hip.so")
WNCC_HEADER = Header.read("diffdrr_wncc_hip.h", "ddrr_wncc", WNCC_ABI_VERSION)
_WNCC_SIGNATURES, _WNCC_RESTYPES, WNCC_EXPORTS = WNCC_HEADER.tables()
WNCC_GROUP_RAYS, WNCC_STATS, WNCC_SLOT_BYTES, WNCC_MAX_POSES = WNCC_HEADER.constants(
    "GROUP_RAYS", "STATS", "SLOT_BYTES", "MAX_POSES")


def wncc_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_wncc_hip.h."""
    return DdrrLibrary(path, WNCC_HEADER)


_wncc_lib: DdrrLibrary | None = None


def get_wncc_lib() -> DdrrLibrary:
    """The weighted NCC library, loaded on first use.  Raises if it has not been built."""
    global _wncc_lib
    if _wncc_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(WNCC_LIB_PATH):
            raise RuntimeError(
                f"{WNCC_LIB_PATH} is missing: the weighted NCC kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _wncc_lib = wncc_library(WNCC_LIB_PATH)
    return _wncc_lib


# ----------------------------------------------------------------- libdiffdrr_wlm_hip.so
# Levenberg-Marquardt registration with a per-pixel weight: the weighted normal-equations sums and the step
# (C ABI: include/diffdrr_wlm_hip.h)
WLM_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_wlm_hip.so")
WLM_HEADER = Header.read("diffdrr_wlm_hip.h", "ddrr_wlm", WLM_ABI_VERSION)
_WLM_SIGNATURES, _WLM_RESTYPES, WLM_EXPORTS = WLM_HEADER.tables()
WLM_SUMS, WLM_GROUP_RAYS, WLM_STATE_DOUBLES, WLM_MAX_POSES = WLM_HEADER.constants(
    "SUMS", "GROUP_RAYS", "STATE_DOUBLES", "MAX_POSES")


def wlm_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_wlm_hip.h."""
    return DdrrLibrary(path, WLM_HEADER)


_wlm_lib: DdrrLibrary | None = None


def get_wlm_lib() -> DdrrLibrary:
    """The weighted Levenberg-Marquardt library, loaded on first use.  Raises if it has not been built."""
    global _wlm_lib
    if _wlm_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(WLM_LIB_PATH):
            raise RuntimeError(
                f"{WLM_LIB_PATH} is missing: the weighted Levenberg-Marquardt kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _wlm_lib = wlm_library(WLM_LIB_PATH)
    return _wlm_lib


# ----------------------------------------------------------------- libdiffdrr_mvlm_hip.so
# multi-view (biplane) Levenberg-Marquardt registration: the rays of S starts seen from V views, the sums of the
# S * V poses and the step on the sums added over a start's views (C ABI: include/diffdrr_mvlm_hip.h)
MVLM_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_mvlm_hip.so")
MVLM_HEADER = Header.read("diffdrr_mvlm_hip.h", "ddrr_mvlm", MVLM_ABI_VERSION)
_MVLM_SIGNATURES, _MVLM_RESTYPES, MVLM_EXPORTS = MVLM_HEADER.tables()
MVLM_SUMS, MVLM_GROUP_RAYS, MVLM_STATE_DOUBLES, MVLM_MAX_POSES = MVLM_HEADER.constants(
    "SUMS", "GROUP_RAYS", "STATE_DOUBLES", "MAX_POSES")


def mvlm_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_mvlm_hip.h."""
    return DdrrLibrary(path, MVLM_HEADER)


_mvlm_lib: DdrrLibrary | None = None


def get_mvlm_lib() -> DdrrLibrary:
    """The multi-view Levenberg-Marquardt library, loaded on first use.  Raises if it has not been built."""
    global _mvlm_lib
    if _mvlm_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(MVLM_LIB_PATH):
            raise RuntimeError(
                f"{MVLM_LIB_PATH} is missing: the multi-view Levenberg-Marquardt kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _mvlm_lib = mvlm_library(MVLM_LIB_PATH)
    return _mvlm_lib


# ----------------------------------------------------------------- libdiffdrr_wmvlm_hip.so
# multi-view Levenberg-Marquardt registration with a pixel weight and a detector per view: the rays, the weighted
# sums of the S * V poses and the step on the sums added over a start's non-empty views
# (C ABI: include/diffdrr_wmvlm_hip.h)
WMVLM_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_wmvlm_hip.so")
WMVLM_HEADER = Header.read("diffdrr_wmvlm_hip.h", "ddrr_wmvlm", WMVLM_ABI_VERSION)
_WMVLM_SIGNATURES, _WMVLM_RESTYPES, WMVLM_EXPORTS = WMVLM_HEADER.tables()
WMVLM_SUMS, WMVLM_GROUP_RAYS, WMVLM_STATE_DOUBLES, WMVLM_MAX_POSES = WMVLM_HEADER.constants(
    "SUMS", "GROUP_RAYS", "STATE_DOUBLES", "MAX_POSES")


def wmvlm_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_wmvlm_hip.h."""
    return DdrrLibrary(path, WMVLM_HEADER)


_wmvlm_lib: DdrrLibrary | None = None


def get_wmvlm_lib() -> DdrrLibrary:
    """The weighted multi-view Levenberg-Marquardt library, loaded on first use.  Raises if it has not been built."""
    global _wmvlm_lib
    if _wmvlm_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(WMVLM_LIB_PATH):
            raise RuntimeError(
                f"{WMVLM_LIB_PATH} is missing: the weighted multi-view Levenberg-Marquardt kernels have not been "
                "built. Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _wmvlm_lib = wmvlm_library(WMVLM_LIB_PATH)
    return _wmvlm_lib


# ----------------------------------------------------------------- libdiffdrr_wmi_hip.so
# MutualInformation under per-pixel weights (C ABI: include/diffdrr_wmi_hip.h): a library of its own next to
# libdiffdrr_mi_hip.so, which stays as it is
WMI_LIB_PATH = os.path.join(_HERE, "csrc", "libdiffdrr_wmi_hip.so")
WMI_HEADER = Header.read("diffdrr_wmi_hip.h", "ddrr_wmi", WMI_ABI_VERSION)
_WMI_SIGNATURES, _WMI_RESTYPES, WMI_EXPORTS = WMI_HEADER.tables()
WMI_MAX_BINS, = WMI_HEADER.constants("MAX_BINS")


def wmi_library(path: str) -> DdrrLibrary:
    """Load and check a build of include/diffdrr_wmi_hip.h."""
    return DdrrLibrary(path, WMI_HEADER)


_wmi_lib: DdrrLibrary | None = None


def get_wmi_lib() -> DdrrLibrary:
    """The weighted MutualInformation library, loaded on first use.  Raises if it has not been built."""
    global _wmi_lib
    if _wmi_lib is None:
        import torch  # noqa: F401  (must own the HIP runtime before we bind to it)

        if not os.path.exists(WMI_LIB_PATH):
            raise RuntimeError(
                f"{WMI_LIB_PATH} is missing: the weighted MutualInformation kernels have not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        _wmi_lib = wmi_library(WMI_LIB_PATH)
    return _wmi_lib
