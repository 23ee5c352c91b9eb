"""Tensor-level entry points over the C ABI: validate, allocate, launch.

Every function takes CUDA(HIP) fp32 tensors, launches on torch's current
stream and returns without synchronising.  CPU tensors are rejected loudly --
this package renders on the MI355X only.
"""
from __future__ import annotations

import ctypes
import os
import weakref

import torch

from . import _lib
from ._lib import REDUCE_MAX, REDUCE_SUM, SIDDON_AUX, TRI_AUX_PLANES

_REDUCE = {"sum": REDUCE_SUM, "max": REDUCE_MAX}
_LOOKUP = {"step": _lib.LOOKUP_STEP, "mid_nearest": _lib.LOOKUP_MID_NEAREST,
           "mid_trilinear": _lib.LOOKUP_MID_TRILINEAR}


def reduce_code(reducefn) -> int:
    if isinstance(reducefn, str) and reducefn in _REDUCE:
        return _REDUCE[reducefn]
    if callable(reducefn):
        raise NotImplementedError(
            "the fused kernels reduce with 'sum' or 'max'; a callable reducefn is served by the "
            "renderer modules through the materialised per-segment / per-sample tensors "
            "(ops.siddon_segments, ops.trilinear_samples)")
    raise ValueError(f"Only supports reducefn 'sum' or 'max', not {reducefn}")


def default_tile() -> tuple[int, int]:
    """(tile_h, tile_w) of the 64 detector pixels one wavefront renders; override
    with DDRR_TILE=HxW.  Rows map to the volume's fastest axis in the usual AP /
    lateral geometry, so the default tile is tall."""
    env = os.environ.get("DDRR_TILE")
    if env:
        h, w = (int(v) for v in env.lower().split("x"))
        if h * w != 64:
            raise ValueError("DDRR_TILE must multiply to 64")
        return h, w
    return 16, 4


def _ptr(t):
    return None if t is None else t.data_ptr()


def on_device(t) -> bool:
    """Whether `t` lives where the kernels run (the tests' host emulation patches this)."""
    return t.is_cuda


def _require_gpu(volume):
    if not volume.is_cuda:
        raise RuntimeError(
            "diffdrr_amd renders on the MI355X only: got a CPU volume tensor (there is no CPU "
            "fallback; move the module with .to('cuda'))."
        )


def _launch(name, device, *args):
    """One asynchronous C-ABI call on torch's current stream of `device`.  (The raw stream handle and the
    device switch only where the current device is another one: `torch.cuda.device(...)` +
    `torch.cuda.current_stream()` cost ~10 us of host time per call -- a third of what an eager
    registration iteration's six launches spend on the host, tools/eager_registration_loop.py.)"""
    _launch_on(_lib.get_lib(), name, device, args)


def _launch_on(lib, name, device, args):
    """:func:`_launch` through the loaded library `lib` (the MutualInformation kernels have their own)."""
    index = device.index
    current = torch.cuda.current_device()
    if index is None or index == current:
        lib.call(name, *args, torch._C._cuda_getCurrentRawStream(current))
        return
    with torch.cuda.device(index):
        lib.call(name, *args, torch._C._cuda_getCurrentRawStream(index))


def _query(name, *args):
    """A C-ABI entry that returns a size (no launch, no stream)."""
    return _lib.get_lib().query(name, *args)


def launch_workspace(shape, device):
    """This launch's own device scratch for a ``*_bricks`` entry point (include/diffdrr_hip.h
    ``launch_ws``: the brick counter and the hand-out order of the bricks).  From torch's caching
    allocator, so it is recycled in stream order, a captured graph gets a block of its private
    pool for as long as the graph lives, and launches on different streams never share one."""
    n = int(_query("ddrr_brick_launch_workspace_bytes", *(int(d) for d in shape)))
    return torch.empty((n + 3) // 4, dtype=torch.int32, device=device)


def _check_rays(volume, source, target, img, dtype=torch.float32):
    _require_gpu(volume)
    for name, t in (("volume", volume), ("source", source), ("target", target), ("img", img)):
        if t is None:
            continue
        if t.dtype != dtype:
            raise NotImplementedError(
                f"{name} must be {dtype} here (got {t.dtype}): the tuned kernels are fp32 like the "
                "reference's default; float64 modules render through the *_f64 entry points")
        if t.device != volume.device:
            raise RuntimeError(f"{name} is on {t.device}, volume on {volume.device}")
    if volume.dim() != 3:
        raise ValueError(f"volume must be (Dx, Dy, Dz), got {tuple(volume.shape)}")
    if target.dim() != 3 or target.shape[-1] != 3:
        raise ValueError(f"target must be (B, N, 3), got {tuple(target.shape)}")
    B, N, _ = target.shape
    if source.dim() != 3 or source.shape[0] != B or source.shape[2] != 3 or \
            source.shape[1] not in (1, N):
        raise ValueError(f"source must be (B, 1, 3) or (B, N, 3), got {tuple(source.shape)}")
    if img is not None and img.numel() != B * N:
        raise ValueError(f"img must have B*N = {B * N} elements, got {tuple(img.shape)}")
    return B, N


class _Rays:
    """The rays of one launch as contiguous tensors -- the caller's own where they are contiguous,
    copies where not -- and, through :meth:`ptr`, every further tensor the launch reads.  Each copy stays
    referenced with the batch until the launch has been enqueued: the autograd nodes hand back the ray
    tensors they were given (a chunk of a (B, N, 3) target is a strided view), and a copy freed before
    its launch is memory that the next allocation may take and overwrite first.  Unchecked (the callers
    of the entries without a volume check what they need); :func:`_rays` checks them first."""
    __slots__ = ("B", "N", "source", "target", "img", "_held")

    def __init__(self, source, target, img):
        self.B, self.N, _ = target.shape
        self.source, self.target = source.contiguous(), target.contiguous()
        self.img = None if img is None else img.contiguous()
        self._held = []

    def ptr(self, t):
        """The device pointer of `t` made contiguous (None for None), held with the batch."""
        if t is None:
            return None
        t = t.contiguous()
        self._held.append(t)
        return t.data_ptr()

    def vol(self, volume):
        """The ABI's (volume, dx, dy, dz) run."""
        return (self.ptr(volume), *volume.shape)

    def rays(self):
        """The ABI's (source, src_n, target, img) run of the per-ray entries."""
        return self.source.data_ptr(), self.source.shape[1], self.target.data_ptr(), _ptr(self.img)

    def grid(self):
        """The (source, target, img) run of the brick entries (one source per pose: no src_n)."""
        return self.source.data_ptr(), self.target.data_ptr(), _ptr(self.img)


def _rays(volume, source, target, img, dtype=torch.float32) -> _Rays:
    """:func:`_check_rays`, then the batch."""
    _check_rays(volume, source, target, img, dtype)
    return _Rays(source, target, img)


def _grid(det, N, source):
    """(det_h, det_w) of a brick launch, whose rays must be one source per pose and an H x W >= 2 x 2
    detector grid."""
    H, W = int(det[0]), int(det[1])
    if H * W != N or source.shape[1] != 1 or min(H, W) < 2:
        raise ValueError("the brick path needs one source per pose and an H*W >= 2x2 ray grid")
    return H, W


def _channels(grad_out, B, N):
    """C of a channel render's gradient grad_out (B, C, N)."""
    C = grad_out.shape[1]
    if grad_out.shape != (B, C, N):
        raise ValueError(f"grad_out must be (B, C, N) = ({B}, C, {N}), got {tuple(grad_out.shape)}")
    return C


def _check_labels(labels_u8, volume=None):
    """A uint8 label map of the volume's shape (any 3-D one for the entries that take no volume)."""
    if volume is None:
        if labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3:
            raise ValueError("labels must be a 3-D uint8 tensor")
    elif labels_u8.dtype != torch.uint8 or labels_u8.shape != volume.shape:
        raise ValueError("labels must be a uint8 tensor of the volume's shape")


def _grad_buffers(B, N, dtype, device, *, rays, img, alpha=None, volume_shape=None, new=torch.empty):
    """The outputs of a backward entry, in the ABI's order, None where not asked: g_source and g_target
    (B, N, 3) per ray with `rays`, g_img (B, N) with `img`, g_alpha (B, N, 2) with `alpha` (the Siddon
    entries have none: alpha=None leaves the key out), g_volume zero-filled (the kernels accumulate into
    it) where a `volume_shape` is given.  `new`: torch.empty, or torch.zeros for kernels that accumulate
    the per-ray outputs too."""
    def buf(want, *shape):
        return new(*shape, dtype=dtype, device=device) if want else None

    g = {"g_source": buf(rays, B, N, 3), "g_target": buf(rays, B, N, 3), "g_img": buf(img, B, N)}
    if alpha is not None:
        g["g_alpha"] = buf(alpha, B, N, 2)
    g["g_volume"] = None if volume_shape is None else \
        torch.zeros(tuple(volume_shape), dtype=dtype, device=device)
    return g


def _batch_grad(g_out, B):
    """(g_out, g_stride) of the gradient of B per-pose values: (B) values with stride 1, or one value for
    the whole batch with stride 0, read in place (the gradient of a summed objective: a 0-dim tensor, or
    what autograd expands it to)."""
    if g_out.dim() == 0 or (g_out.dim() == 1 and B > 1 and g_out.stride(0) == 0):
        return g_out, 0
    return g_out.contiguous(), 1


def _empty(B, N):
    """Nothing to render (an empty batch has no valid device pointers to hand over)."""
    return B == 0 or N == 0


def rays_form_detector_grid(source, target, det_h, det_w, tol=2e-3) -> bool:
    """Whether ``target`` (B, det_h * det_w, 3) is, per pose, the row-major affine grid
    ``t00 + i e_i + j e_j`` the volume-stationary kernels assume (they cull candidate rays with
    that model; rays that do not follow it would be dropped silently), within ``tol`` voxels.
    One fused reduction and ONE host sync: meant for ray lists of unknown provenance
    (``DRR.render`` called directly); rays that come out of ``Detector.forward`` are such a grid
    by construction (reference detector.py:126, 147-153) and are not checked."""
    B, N, _ = target.shape
    if N != det_h * det_w or min(det_h, det_w) < 2 or source.shape[1] != 1:
        return False
    if target.numel() == 0:
        return False  # (an empty batch: the per-ray entry points return empty results)
    t = target.detach().reshape(B, det_h, det_w, 3)
    t00 = t[:, :1, :1]
    ei = (t[:, -1:, :1] - t00) / (det_h - 1)
    ej = (t[:, :1, -1:] - t00) / (det_w - 1)
    i = torch.arange(det_h, device=t.device, dtype=t.dtype).view(1, det_h, 1, 1)
    j = torch.arange(det_w, device=t.device, dtype=t.dtype).view(1, 1, det_w, 1)
    dev = (t00 + i * ei + j * ej - t).abs().amax()
    # a grid, not a line or a point: the pixel steps span a plane (|e_i x e_j| well above the
    # tolerance; all targets equal, or all on one line, is not a detector)
    area = torch.linalg.cross(ei.reshape(B, 3), ej.reshape(B, 3)).norm(dim=-1).amin()
    return bool(((dev <= tol) & (area > tol * tol)).item())


def _hints(det, tile, N):
    if det is None or det[0] * det[1] != N:
        return 0, 0, 1, 64
    th, tw = default_tile() if tile is None else tile
    return int(det[0]), int(det[1]), int(th), int(tw)


def siddon_forward(volume, source, target, img, *, voxel_shift=0.5, eps=1e-8, reducefn="sum",
                   lookup="step", align_corners=False, want_aux=False, count_voxels=False,
                   det=None, tile=None):
    """-> (out (B,N), aux (B,N,8) | None, n_vox (B,N) int32 | None)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    out = torch.empty(B, N, dtype=torch.float32, device=volume.device)
    aux = torch.empty(B, N, SIDDON_AUX, dtype=torch.float32, device=volume.device) \
        if want_aux else None
    nvox = torch.empty(B, N, dtype=torch.int32, device=volume.device) if count_voxels else None
    hints = _hints(det, tile, N)
    if _empty(B, N):
        return out, aux, nvox
    _launch(
        "ddrr_siddon_forward", volume.device, *r.vol(volume), *r.rays(), B, N, float(voxel_shift), float(eps),
        reduce_code(reducefn), _LOOKUP[lookup], int(bool(align_corners)), *hints,
        out.data_ptr(), _ptr(aux), _ptr(nvox))
    return out, aux, nvox


_vmax_cache = {}  # id(volume) -> (weakref to the volume, its version, max |volume|)


def volume_absmax(volume) -> float:
    """max |volume| as a host float, cached per volume TENSOR (weak reference + version, so a
    different volume at a recycled address is never confused with it): the scale of the
    packed backward record.  One reduction and one host sync when the volume changes."""
    ent = _vmax_cache.get(id(volume))
    if ent is not None and ent[0]() is volume and ent[1] == volume._version:
        return ent[2]
    value = float(volume.detach().abs().max().item())
    key = id(volume)
    _vmax_cache[key] = (weakref.ref(volume, lambda _, k=key: _vmax_cache.pop(k, None)),
                        volume._version, value)
    return value


def record_blocks(B, N) -> int:
    """16-ray blocks of the brick kernel's float backward record (csrc/record_layout.h)."""
    return -(-(B * N) // _lib.REC_BLOCK_RAYS)


def _aux_layout(aux, B, N):
    if aux.shape == (B, N, SIDDON_AUX):
        return _lib.AUX_INTERLEAVED
    if aux.shape == (record_blocks(B, N), _lib.REC_BLOCK_FLOATS):
        return _lib.AUX_BLOCKED
    if aux.shape == (_lib.PACKED_AUX_PLANES, B, N):
        return _lib.AUX_PACKED
    raise ValueError(f"aux has shape {tuple(aux.shape)}: neither (B,N,8), the blocked record "
                     f"(ceil(B N / 16), 80) nor the packed one (7,B,N)")


def record_planes(aux, B, N):
    """The blocked float record of :func:`siddon_forward_bricks` as (5, B, N) planes
    I, S0x, S0z, S1x, S1z (a copy; for inspection and tests)."""
    R = B * N
    blk = aux.reshape(-1, 5, 16)  # lines: [g0 p0|p1] [g0 p2|p3] [g1 p0|p1] [g1 p2|p3] [p4 x16]
    pairs = blk[:, :4].reshape(-1, 2, 2, 2, 8)        # block, group, line of group, plane in line, ray
    p03 = pairs.permute(2, 3, 0, 1, 4).reshape(4, -1)  # plane = 2 * line + plane-in-line
    return torch.cat([p03, blk[:, 4].reshape(1, -1)])[:, :R].reshape(5, B, N)


_BRICK_STORAGE = {"f32": _lib.BRICKS_F32, "q16": _lib.BRICKS_Q16, "q16p": _lib.BRICKS_Q16_PACKED,
                  "q16y": _lib.BRICKS_Q16_Y, "q16py": _lib.BRICKS_Q16_PACKED_Y}
# the same storage on bricks whose long axis is y (32 x 64 x 32 instead of 32 x 32 x 64): a workspace of
# its own -- the brick grid and the packed images differ with the shape
_Y_TWIN = {"q16": "q16y", "q16p": "q16py"}
_range_cache = {}  # (id(volume), storage) -> _Workspace; the storage's name carries the bricks' shape
_launches = 0      # brick launches on a 16-bit storage so far (stamps _Workspace.used)


class _Workspace:
    """Cache entry of :func:`brick_workspace`: the buffer and what it was built from."""
    __slots__ = ("ref", "buf", "built_version", "built_ptr", "churn", "event", "stream", "used")

    def __init__(self, ref, buf):
        self.ref, self.buf = ref, buf
        self.built_version = None  # volume._version the buffer holds the bricks of (None: nothing)
        self.built_ptr = None      # ... and the address of the storage they were read from
        self.churn = 0             # rebuilds because the volume had changed
        self.event = self.stream = None  # end of the building launch, and the stream it ran on
        self.used = 0              # the last launch that rendered from it (_launches)


def _workspace_entry(volume, storage):
    ent = _range_cache.get((id(volume), storage))
    if ent is not None and ent.ref() is volume and ent.buf.device == volume.device:
        return ent
    return None


def _used_entry(volume, storage):
    """The entry the reporting functions mean by "q16" / "q16p": of the two shapes' workspaces of this
    volume (``_Y_TWIN``), the one a launch rendered from last -- the renderer chooses the shape
    (``Siddon.brick_axis``), its callers ask by the storage's name."""
    ents = [e for e in (_workspace_entry(volume, s) for s in (storage, _Y_TWIN.get(storage))) if e is not None]
    return max(ents, key=lambda e: e.used) if ents else None


def brick_workspace(volume, storage="q16"):
    """Workspace of the 16-bit brick staging (include/diffdrr_hip.h DDRR_BRICKS_Q16 /
    _PACKED): a header, the bricks' (min, max) and fp32-fallback flags and, for "q16p", the
    bricks themselves as they lie in LDS (+52 % of the volume's bytes, held as long as the volume
    tensor lives).  Cached per volume TENSOR and storage; "q16y" / "q16py" are the same storages on
    32 x 64 x 32 bricks, each a workspace of its own.  The kernel fills it on the first
    launch after the volume changed (one pass over the volume); the launch that filled it
    reports so with :func:`brick_workspace_commit`, and only then do later calls get
    ``valid`` = 1 -- a call that returns early (empty batch) or fails leaves it unbuilt.
    "Changed" is what PyTorch itself tracks: the tensor's version counter (any in-place op,
    ``no_grad`` or not) and the address of its storage (``volume.data = other``).  In-place edits
    that bypass the version counter -- ``volume.data[...] = x``, ``volume.data.copy_(x)`` -- are
    caught ON THE DEVICE: the workspace carries a fingerprint of the volume it was built from (1024
    voxels spread over it, csrc/brick_core.h) and a launch that finds it changed renders every
    brick from the volume's own fp32 values -- slower, never stale
    (:func:`brick_workspace_stale` reports it; :func:`invalidate_brick_workspace` /
    ``Siddon.volume_changed`` rebuild).  Only an edit of a few voxels that misses all 1024 samples
    needs the explicit call.
    -> (tensor, valid)"""
    key = (id(volume), storage)
    ent = _workspace_entry(volume, storage)
    n = (int(_query("ddrr_brick_workspace_bytes", *(int(d) for d in volume.shape),
                    _BRICK_STORAGE[storage])) + 3) // 4
    if ent is None or ent.buf.numel() != n:
        # (a volume edited in place keeps its buffer: a captured graph may hold the address)
        ent = _Workspace(weakref.ref(volume, lambda _, k=key: _range_cache.pop(k, None)),
                         torch.empty(n, dtype=torch.float32, device=volume.device))
        _range_cache[key] = ent
    valid = int(ent.built_version is not None and ent.built_version == volume._version
                and ent.built_ptr == volume.data_ptr())
    if valid and ent.event is not None and not torch.cuda.is_current_stream_capturing():
        # built on another stream: this stream's launches must not overtake the build
        if ent.event.query():
            ent.event = ent.stream = None
        elif torch.cuda.current_stream(volume.device) != ent.stream:
            torch.cuda.current_stream(volume.device).wait_event(ent.event)
    return ent.buf, valid


def brick_workspace_commit(volume, storage):
    """The launch that was handed ``valid`` = 0 has been enqueued: the workspace now holds (in
    stream order) the bricks of the volume's current version."""
    ent = _workspace_entry(volume, storage)
    if ent is None or (ent.built_version == volume._version and ent.built_ptr == volume.data_ptr()):
        return
    if volume.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        # a captured launch has not run: the workspace stays unbuilt for eager launches (which
        # rebuild into the same buffer); the captured graph rebuilds it on every replay
        return
    if ent.built_version is not None:
        ent.churn += 1  # workspace_churn() lets the renderer stop paying for rebuilds
    ent.built_version = volume._version
    ent.built_ptr = volume.data_ptr()
    ent.event = ent.stream = None
    if volume.device.type == "cuda":
        ent.stream = torch.cuda.current_stream(volume.device)
        ent.event = torch.cuda.Event()
        ent.event.record(ent.stream)


def invalidate_brick_workspace(volume):
    """The volume was edited in a way PyTorch does not track (``volume.data[...] = x``): the next
    render rebuilds its cached 16-bit bricks (every storage).  Without this call such an edit is
    still rendered correctly -- the launch notices (:func:`brick_workspace`) and takes the fp32
    path for every brick -- but at the fp32 bricks' speed until the workspace is rebuilt."""
    for storage in ("q16", "q16p", "q16y", "q16py"):
        ent = _workspace_entry(volume, storage)
        if ent is not None:
            ent.built_version = ent.built_ptr = None


def brick_workspace_stale(volume, storage):
    """How many launches found the volume changed under this built workspace (its fingerprint did
    not match: they rendered from the fp32 values); 0 for a workspace in step with its volume, None
    if none is built.  Reads one word from the device (a host sync).  "q16" / "q16p": of the shape last
    rendered from (``_used_entry``)."""
    ent = _used_entry(volume, storage)
    if ent is None or ent.built_version is None:
        return None
    return int(ent.buf[2:3].view(torch.int32).item())


def workspace_churn(volume, storage):
    """How many times the workspace of this volume was rebuilt because the volume had changed
    (0: built once): a volume that changes between renders gains nothing from a packed copy.
    "q16" / "q16p": of the shape last rendered from (``_used_entry``)."""
    ent = _used_entry(volume, storage)
    return ent.churn if ent is not None else 0


def brick_fallbacks(volume, storage):
    """(bricks rendered from their own fp32 values, bricks) of the built workspace of this
    volume -- the 16-bit block quantisation is only used for bricks whose range is small against
    their level (csrc/brick_step.h q16_usable) -- or None if no launch has built it yet.
    Reads two words from the device (a host sync).  "q16" / "q16p" report the workspace a launch
    rendered from last, whichever shape its bricks have (``_used_entry``: 32 x 32 x 64, or 32 x 64 x 32 where
    ``Siddon.brick_axis`` chose "y"); "q16y" / "q16py" name the y-long one."""
    ent = _used_entry(volume, storage)
    if ent is None or ent.built_version is None:
        return None
    head = ent.buf[:2].view(torch.int32).tolist()
    return head[0], head[1]


def brick_storage_applies(volume) -> bool:
    """Whether the 16-bit brick storages can serve this volume tensor at all: a non-contiguous
    volume is a new temporary on every call (its workspace would be rebuilt -- and its memory
    churned -- per render).  Any shape of at least four slices does (the reference's example CT has
    133: the staging reads quads of four voxels from dword-aligned addresses); a thinner volume is
    rendered from its fp32 values by the general brick kernel whatever the storage
    (csrc/bricks_fwd.hip launch_fwd_bricks, csrc/brick_core.h quads_serve), which builds no
    workspace: handing it one would leave :func:`brick_fallbacks` and :func:`brick_workspace_stale`
    reading words no launch has written."""
    return volume.dim() == 3 and volume.is_contiguous() and volume.numel() >= 4 and volume.shape[2] >= 4


def brick_ranges(volume):
    """(kept name) the "q16" workspace of :func:`brick_workspace`"""
    return brick_workspace(volume, "q16")


def brick_record_buffer(B, N, device):
    """The (uninitialised) blocked float record of a brick launch of B x N rays."""
    return torch.empty(record_blocks(B, N), _lib.REC_BLOCK_FLOATS, dtype=torch.float32, device=device)


def siddon_forward_bricks(volume, source, target, img, det, *, voxel_shift=0.5, eps=1e-8,
                          want_aux=False, record_vmax=0.0, storage="f32", want_image=True,
                          aux=None, out=None, launch_ws=None, cleared=False, pixel_mask=None, axis="z"):
    """Detector-grid Siddon (sum) through the volume-stationary brick kernel: every 32^3
    brick is staged in LDS once and all rays of all poses are traced through it.
    Requires the targets to be the affine detector grid DRR builds.
    -> (out (B,N), aux | None); aux is the blocked float record (ceil(B N / 16), 80)
    (csrc/record_layout.h; :func:`record_planes` unpacks it), or with ``record_vmax`` =
    max |volume| > 0 the (7,B,N) packed fixed-point record (3 atomics per ray and brick
    instead of 5, bit-reproducible; csrc/record_pack.h).
    ``storage``: "f32" stages the volume's own values in 32^3 bricks, "q16" a 16-bit block
    quantisation in 32 x 32 x 64 bricks, "q16p" the same bricks from a packed copy kept in the
    cached workspace (include/diffdrr_hip.h DDRR_BRICKS_*).  ``axis`` = "y": the 16-bit storages on
    32 x 64 x 32 bricks ("q16y" / "q16py", which can also be named directly; a workspace of their own) --
    fewer (ray, brick) pairs where the rays run along y; on the device only (a CPU tensor, i.e. the host
    emulation, keeps the z-long bricks), and without meaning for "f32".
    ``aux`` / ``out`` / ``launch_ws``: a record (:func:`brick_record_buffer`) or an image (B, N) and a
    launch workspace (:func:`launch_workspace`) the caller brings along; ``cleared``: what the
    launch's atomics add to (the record if one is wanted, else the image) and the workspace's
    counter are zero already (:func:`pose_raygen_forward` did it in its launch) -- the call then
    clears nothing.  ``pixel_mask``: an int32 tensor of ceil(N / 32) words, one bit per pixel of the
    grid (:func:`pixel_mask_of`): only the pixels whose bit is set are rendered, image and record
    hold zeros at the others (``p_subsample``: reference drr.py:36-39, 142-147)."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    H, W = _grid(det, N, source)
    if storage != "f32" and not brick_storage_applies(volume):
        storage = "f32"
    if axis not in ("y", "z"):
        raise ValueError(f"axis must be 'y' or 'z', not {axis!r}")
    if axis == "y" and volume.device.type == "cuda":
        storage = _Y_TWIN.get(storage, storage)
    # (want_image = False with want_aux: the record alone -- siddon_ncc_forward forms the image)
    need_out = want_image or not want_aux
    if out is not None and (not need_out or out.shape != (B, N) or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != volume.device):
        raise ValueError("out: a contiguous float32 (B, N) image on the volume's device, where one is written")
    if need_out and out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=volume.device)
    ranges, valid = brick_workspace(volume, storage) if storage != "f32" else (None, 0)
    packed = bool(want_aux and record_vmax and record_vmax > 0.0)
    if cleared and (launch_ws is None or packed or (want_aux and aux is None)):
        raise ValueError("cleared=True: the float record (an image with it is formed from the record afterwards) "
                         "or the image, and the launch workspace, as the caller cleared them")
    if want_aux and aux is None:
        shape = (_lib.PACKED_AUX_PLANES, B, N) if packed else \
            (record_blocks(B, N), _lib.REC_BLOCK_FLOATS)
        aux = torch.empty(*shape, dtype=torch.float32, device=volume.device)
    elif not want_aux:
        aux = None
    if _empty(B, N):
        return out, aux
    if launch_ws is None:
        launch_ws = launch_workspace(volume.shape, volume.device)
    if pixel_mask is not None and (pixel_mask.dtype != torch.int32 or pixel_mask.numel() != (N + 31) // 32
                                   or not pixel_mask.is_contiguous() or pixel_mask.device != volume.device):
        raise ValueError("pixel_mask: a contiguous int32 tensor of ceil(N / 32) words on the volume's device")
    _launch(
        "ddrr_siddon_forward_bricks" if pixel_mask is None else "ddrr_siddon_forward_bricks_masked",
        volume.device, *r.vol(volume), *r.grid(), B, H, W, float(voxel_shift), float(eps),
        _ptr(out), _ptr(aux), float(record_vmax) if packed else 0.0,
        _BRICK_STORAGE[storage], _ptr(ranges), int(valid) | (_lib.BRICKS_CLEARED if cleared else 0),
        launch_ws.data_ptr(), *(() if pixel_mask is None else (pixel_mask.data_ptr(),)))
    if storage != "f32":
        global _launches
        _launches += 1
        _workspace_entry(volume, storage).used = _launches
        if not valid:
            brick_workspace_commit(volume, storage)
    return out, aux


def pixel_mask_of(index, n_pixels):
    """One bit per pixel of a detector grid of ``n_pixels`` pixels, set for the pixels listed in
    ``index`` (int64 tensor): the ``pixel_mask`` of :func:`siddon_forward_bricks`, int32 words on
    ``index``'s device."""
    words = torch.zeros((n_pixels + 31) // 32 * 32, dtype=torch.bool, device=index.device)
    words[index] = True
    weights = (1 << torch.arange(32, dtype=torch.int64, device=index.device))
    packed = (words.view(-1, 32).to(torch.int64) * weights).sum(dim=1)
    return (packed - ((packed >> 31) << 32)).to(torch.int32).contiguous()  # (two's complement words)


def siddon_backward_rays(aux, grad_out, source, target, img, *, eps=1e-8, reducefn="sum",
                         want_img_grad=True):
    """aux: (B,N,8) interleaved record (generic forward) or the blocked / packed record of
    the brick forward.  -> (g_source (B,N,3) per ray, g_target (B,N,3), g_img (B,N) | None)"""
    B, N, _ = target.shape
    layout = _aux_layout(aux, B, N)
    g_source = torch.empty(B, N, 3, dtype=torch.float32, device=target.device)
    g_target = torch.empty(B, N, 3, dtype=torch.float32, device=target.device)
    g_img = torch.empty(B, N, dtype=torch.float32, device=target.device) if want_img_grad else None
    if not _empty(B, N):
        r = _Rays(source, target, img)
        _launch(
            "ddrr_siddon_backward_rays", target.device, aux.data_ptr(), layout, r.ptr(grad_out), *r.rays(), B, N,
            float(eps), reduce_code(reducefn), g_source.data_ptr(), g_target.data_ptr(), _ptr(g_img))
    return g_source, g_target, g_img


def pose_euler_forward(rot, xyz, axes, reorient34):
    """rot, xyz (B,3) radians / world units; axes: 3 ints in {0,1,2}; reorient34 (3,4).
    -> Mw (B,3,4) = [R | R xyz] @ reorient"""
    _require_gpu(rot)
    B = rot.shape[0]
    rot, xyz, reorient34 = rot.contiguous(), xyz.contiguous(), reorient34.contiguous()
    Mw = torch.empty(B, 3, 4, dtype=torch.float32, device=rot.device)
    if B:
        _launch("ddrr_pose_euler_forward", rot.device, rot.data_ptr(), xyz.data_ptr(), *axes,
                reorient34.data_ptr(), B, Mw.data_ptr())
    return Mw


def pose_euler_backward(rot, xyz, axes, reorient34, gMw):
    B = rot.shape[0]
    rot, xyz, reorient34, gMw = (t.contiguous() for t in (rot, xyz, reorient34, gMw))
    g_rot, g_xyz = torch.empty_like(rot), torch.empty_like(xyz)
    if B:
        _launch("ddrr_pose_euler_backward", rot.device, rot.data_ptr(), xyz.data_ptr(), *axes,
                reorient34.data_ptr(), gMw.data_ptr(), B, g_rot.data_ptr(), g_xyz.data_ptr())
    return g_rot, g_xyz


def ncc_forward(x1, x2, eps):
    """x2 (B,N); x1 (B,N) or (1,N) shared by the batch.  -> (ncc (B), stats (B,5))"""
    _require_gpu(x2)
    B, N = x2.shape
    shared = x1.shape[0] == 1 and B != 1
    x1, x2 = x1.contiguous(), x2.contiguous()
    out = torch.empty(B, dtype=torch.float32, device=x2.device)
    stats = torch.empty(B, 5, dtype=torch.float32, device=x2.device)
    if B:
        _launch("ddrr_ncc_forward", x2.device, x1.data_ptr(), 0 if shared else N, x2.data_ptr(), B,
                N, float(eps), out.data_ptr(), stats.data_ptr())
    return out, stats


def ncc_backward(x1, x2, stats, g_out, want_x1, want_x2):
    B, N = x2.shape
    shared = x1.shape[0] == 1 and B != 1
    x1, x2 = x1.contiguous(), x2.contiguous()
    # (the gradient of `.sum()` / `.mean()` arrives as an expanded scalar: read in place, stride 0)
    g_out, g_stride = _batch_grad(g_out, B)
    g_x2 = torch.empty_like(x2) if want_x2 else None
    g_x1 = torch.empty_like(x2) if (want_x1 and not shared) else None
    if B:
        _launch("ddrr_ncc_backward", x2.device, x1.data_ptr(), 0 if shared else N, x2.data_ptr(),
                stats.data_ptr(), g_out.data_ptr(), g_stride, B, N, _ptr(g_x1), _ptr(g_x2))
    return g_x1, g_x2


def ncc_patch_forward(x1, x2, p, eps, want_coef=True):
    """Patch-wise NCC (reference metrics.py:16-44, ``patch_size = p``) of image pairs: x2 (B, H, W);
    x1 (B, H, W) or (1, H, W) shared by the batch.  -> (ncc (B), coef (B, H-p+1, W-p+1, 4) | None: what
    :func:`ncc_patch_backward` needs)"""
    _require_gpu(x2)
    B, H, W = x2.shape
    shared = x1.shape[0] == 1 and B != 1
    x1, x2 = x1.contiguous(), x2.contiguous()
    out = torch.empty(B, dtype=torch.float32, device=x2.device)
    coef = torch.empty(B, H - p + 1, W - p + 1, 4, dtype=torch.float32, device=x2.device) if want_coef else None
    if B:
        _launch("ddrr_ncc_patch_forward", x2.device, x1.data_ptr(), 0 if shared else H * W, x2.data_ptr(), B,
                H, W, int(p), float(eps), out.data_ptr(), _ptr(coef))
    return out, coef


def ncc_patch_backward(x1, x2, coef, g_out, p):
    """d (sum_b g_out[b] ncc[b]) / d x2 (B, H, W) of :func:`ncc_patch_forward`."""
    B, H, W = x2.shape
    shared = x1.shape[0] == 1 and B != 1
    x1, x2 = x1.contiguous(), x2.contiguous()
    g_out, g_stride = _batch_grad(g_out, B)
    g_x2 = torch.empty_like(x2)
    if B:
        _launch("ddrr_ncc_patch_backward", x2.device, x1.data_ptr(), 0 if shared else H * W, x2.data_ptr(),
                coef.data_ptr(), g_out.data_ptr(), g_stride, B, H, W, int(p), g_x2.data_ptr())
    return g_x2


def sobel_forward(img):
    """img (B, H, W) -> (B, 2, H, W): the Sobel x / y responses (reference metrics.py:69-94)."""
    _require_gpu(img)
    B, H, W = img.shape
    img = img.contiguous()
    out = torch.empty(B, 2, H, W, dtype=torch.float32, device=img.device)
    if B:
        _launch("ddrr_sobel_forward", img.device, img.data_ptr(), B, H, W, out.data_ptr())
    return out


def sobel_backward(g_out):
    """Adjoint of :func:`sobel_forward`: g_out (B, 2, H, W) -> (B, H, W)."""
    B, _, H, W = g_out.shape
    g_out = g_out.contiguous()
    g_img = torch.empty(B, H, W, dtype=torch.float32, device=g_out.device)
    if B:
        _launch("ddrr_sobel_backward", g_out.device, g_out.data_ptr(), B, H, W, g_img.data_ptr())
    return g_img


def blur_sobel_forward(img, taps):
    """img (B, H, W) -- or one image expanded over the batch -- -> (B, 2, H, W): the Sobel responses of the
    Gaussian-blurred image (reference metrics.py:66, 88-93) in one launch; taps: (k) on the device."""
    _require_gpu(img)
    B, H, W = img.shape
    shared = B > 1 and img.stride(0) == 0
    if shared:
        img = img[:1]
    img = img.contiguous()
    out = torch.empty(B, 2, H, W, dtype=torch.float32, device=img.device)
    if B:
        _launch("ddrr_blur_sobel_forward", img.device, img.data_ptr(), 0 if shared else H * W, B, H, W,
                taps.data_ptr(), int(taps.numel()), out.data_ptr())
    return out


def blur_sobel_backward(g_out, taps):
    """Adjoint of :func:`blur_sobel_forward`: g_out (B, 2, H, W) -> (B, H, W)."""
    B, _, H, W = g_out.shape
    g_out = g_out.contiguous()
    g_img = torch.empty(B, H, W, dtype=torch.float32, device=g_out.device)
    if B:
        _launch("ddrr_blur_sobel_backward", g_out.device, g_out.data_ptr(), B, H, W, taps.data_ptr(),
                int(taps.numel()), g_img.data_ptr())
    return g_img


def raygen_forward(Mw, Ainv, P):
    """Fused ray generation (detector.py:151-153 + drr.py:201-205).  Mw (B,3,4) world pose
    per DRR, Ainv (3,4) world -> voxel, P (N,3) calibrated detector points.
    -> (source_v (B,1,3), target_v (B,N,3), img (B,N))"""
    _require_gpu(Mw)
    B, N = Mw.shape[0], P.shape[0]
    if Mw.shape[1:] != (3, 4) or Ainv.shape != (3, 4) or P.shape != (N, 3):
        raise ValueError("raygen_forward: Mw (B,3,4), Ainv (3,4), P (N,3) expected")
    for t in (Mw, Ainv, P):
        if t.dtype != torch.float32 or t.device != Mw.device:
            raise NotImplementedError("raygen_forward needs float32 tensors on one device")
    Mw, Ainv, P = Mw.contiguous(), Ainv.contiguous(), P.contiguous()
    dev = Mw.device
    source = torch.empty(B, 1, 3, dtype=torch.float32, device=dev)
    target = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    img = torch.empty(B, N, dtype=torch.float32, device=dev)
    if not _empty(B, N):
        _launch("ddrr_raygen_forward", dev, Mw.data_ptr(), Ainv.data_ptr(), P.data_ptr(), B, N,
                source.data_ptr(), target.data_ptr(), img.data_ptr())
    elif B > 0:
        source.zero_()
    return source, target, img


def siddon_backward_pose(aux, grad_out, source, target, img, Mw, Ainv, P, *, eps=1e-8,
                         with_img_path=True):
    """dLoss/dMw (B,3,4): the renderer's ray gradients chained through the ray generation
    and reduced per pose in one kernel (reduce sum)."""
    B, N, _ = target.shape
    layout = _aux_layout(aux, B, N)
    gMw = torch.empty(B, 3, 4, dtype=torch.float32, device=target.device)  # (zero-filled by the call)
    if B == 0:
        return gMw
    # (named, so that a contiguous copy outlives the launch)
    grad_out, source, target, img = (t.contiguous() for t in (grad_out, source, target, img))
    Mw, Ainv, P = Mw.contiguous(), Ainv.contiguous(), P.contiguous()
    _launch("ddrr_siddon_backward_pose", target.device, aux.data_ptr(), layout,
            grad_out.data_ptr(), source.data_ptr(), target.data_ptr(), img.data_ptr(),
            Mw.data_ptr(), Ainv.data_ptr(), P.data_ptr(), B, N, float(eps),
            int(bool(with_img_path)), gMw.data_ptr())
    return gMw


# ---------------------------------------------------------------- the fused registration step
_ncc_ws = {}  # (device, stream, B) -> workspace of ddrr_siddon_ncc_* (zero between calls)


def _blocked_record_only(name, aux, B, N):
    """The fused step's entries read the blocked record alone (no layout argument in their C ABI): any other
    record, or any other shape, would be misread silently."""
    if _aux_layout(aux, B, N) != _lib.AUX_BLOCKED:
        raise ValueError(f"{name} reads the blocked record (ceil(B N / 16), 80) of siddon_forward_bricks only: "
                         f"aux has shape {tuple(aux.shape)}")


def _fixed_rows(name, x1, B, N):
    if x1.dim() != 2 or x1.shape[1] != N or x1.shape[0] not in (1, B):
        raise ValueError(f"{name}: x1 has shape {tuple(x1.shape)}: ({B}, {N}), or (1, {N}) for one image shared "
                         f"by the batch, expected")


def _pose_chain(Mw, Ainv, P, rot, xyz, axes, reorient34):
    """The pose chain as the entries behind :func:`pose_raygen_forward` take it -> (the contiguous tensors, for the
    caller to hold until its launch; the argument run ``Mw, Ainv, P, rot, xyz, *axes, reorient34``)."""
    Mw, Ainv, P, rot, xyz, reorient34 = held = tuple(t.contiguous() for t in (Mw, Ainv, P, rot, xyz, reorient34))
    return held, (Mw.data_ptr(), Ainv.data_ptr(), P.data_ptr(), rot.data_ptr(), xyz.data_ptr(), *axes,
                  reorient34.data_ptr())


def _pose_grads(B, device):
    """(g_rot, g_xyz): two (B, 3) float32 tensors for an entry to write."""
    return torch.empty(B, 3, dtype=torch.float32, device=device), torch.empty(B, 3, dtype=torch.float32, device=device)


def siddon_ncc_workspace(B, device):
    """The caller-owned accumulators / tickets of :func:`siddon_ncc_forward` and
    :func:`siddon_ncc_backward_pose`: zero when first handed over, left zero by every call, so one
    buffer per (device, stream, batch size) serves every call on that stream without a fill.
    (First use inside a stream capture: the zero-fill becomes a node of the graph -- harmless, one
    small launch per replay; ``GraphedIteration`` creates the buffer for its capture stream before
    it captures.)"""
    dev = torch.device(device)
    sid = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    key = (dev, sid, int(B))
    ws = _ncc_ws.get(key)
    if ws is None:
        n = int(_query("ddrr_siddon_ncc_workspace_bytes", int(B)))
        ws = _ncc_ws[key] = torch.zeros((n + 7) // 8, dtype=torch.float64, device=dev)
    return ws


def pose_raygen_forward(rot, xyz, axes, reorient34, Ainv, P, *, clear=None, clear_launch_ws=None):
    """pose_euler_forward + raygen_forward in one launch -> (Mw (B,3,4), source_v (B,1,3),
    target_v (B,N,3), img (B,N)).  ``clear`` (a float32 tensor) and ``clear_launch_ws`` (the launch
    workspace of the render that follows) are zeroed by the same launch: hand them to
    :func:`siddon_forward_bricks` with ``cleared=True``."""
    _require_gpu(rot)
    B, N = rot.shape[0], P.shape[0]
    rot, xyz, reorient34, Ainv, P = (t.contiguous() for t in (rot, xyz, reorient34, Ainv, P))
    dev = rot.device
    Mw = torch.empty(B, 3, 4, dtype=torch.float32, device=dev)
    source = torch.empty(B, 1, 3, dtype=torch.float32, device=dev)
    target = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    img = torch.empty(B, N, dtype=torch.float32, device=dev)
    if not _empty(B, N):
        _launch("ddrr_pose_raygen_forward", dev, rot.data_ptr(), xyz.data_ptr(), *axes,
                reorient34.data_ptr(), Ainv.data_ptr(), P.data_ptr(), B, N, Mw.data_ptr(),
                source.data_ptr(), target.data_ptr(), img.data_ptr(), _ptr(clear),
                0 if clear is None else clear.numel(), _ptr(clear_launch_ws))
    elif clear is not None or clear_launch_ws is not None:
        raise ValueError("pose_raygen_forward: nothing is launched for an empty batch, nothing is cleared")
    return Mw, source, target, img


def siddon_ncc_forward(aux, img, x1, eps, *, want_image=False, want_sum=False):
    """Per-pose NCC of the fixed image(s) ``x1`` ((B | 1), N) with the DRRs whose blocked record
    is ``aux`` (``img`` (B,N): the rays' lengths): the image is formed from the record on the fly.
    -> (ncc (B), stats (B,5), image (B,N) | None[, sum of the B values (0-dim), with ``want_sum``:
    put together by the same launch])"""
    B, N = img.shape
    _blocked_record_only("siddon_ncc_forward", aux, B, N)
    _fixed_rows("siddon_ncc_forward", x1, B, N)
    shared = x1.shape[0] == 1 and B != 1
    x1, img = x1.contiguous(), img.contiguous()
    dev = img.device
    ncc = torch.empty(B, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 5, dtype=torch.float32, device=dev)
    out = torch.empty(B, N, dtype=torch.float32, device=dev) if want_image else None
    total = (torch.empty((), dtype=torch.float32, device=dev) if B else
             torch.zeros((), dtype=torch.float32, device=dev)) if want_sum else None
    if B:
        _launch("ddrr_siddon_ncc_forward", dev, aux.data_ptr(), img.data_ptr(), x1.data_ptr(),
                0 if shared else N, B, N, float(eps), siddon_ncc_workspace(B, dev).data_ptr(),
                ncc.data_ptr(), stats.data_ptr(), _ptr(out), _ptr(total))
    return (ncc, stats, out, total) if want_sum else (ncc, stats, out)


def pose_adam_step(rot, xyz, g_rot, g_xyz, m_rot, v_rot, m_xyz, v_xyz, step_rot, step_xyz, *, lr_rot, lr_xyz,
                   betas=(0.9, 0.999), eps=1e-8, maximize=False):
    """One Adam step of the two pose parameter groups, in place, in one launch (include/diffdrr_hip.h
    ddrr_pose_adam_step: torch.optim.Adam's update; `step_*` are 1-element float tensors)."""
    _require_gpu(rot)
    B = rot.shape[0]
    for t in (rot, xyz, g_rot, g_xyz, m_rot, v_rot, m_xyz, v_xyz):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != (B, 3):
            raise ValueError("pose_adam_step: contiguous float32 (B, 3) tensors")
    for t in (step_rot, step_xyz):
        if t.dtype != torch.float32 or t.numel() != 1:
            raise ValueError("pose_adam_step: 1-element float32 step counters")
    if B:
        _launch("ddrr_pose_adam_step", rot.device, rot.data_ptr(), xyz.data_ptr(), g_rot.data_ptr(),
                g_xyz.data_ptr(), m_rot.data_ptr(), v_rot.data_ptr(), m_xyz.data_ptr(), v_xyz.data_ptr(),
                step_rot.data_ptr(), step_xyz.data_ptr(), B, float(lr_rot), float(lr_xyz), float(betas[0]),
                float(betas[1]), float(eps), int(bool(maximize)))


def siddon_ncc_backward_pose(aux, img, x1, stats, g_out, source, target, Mw, Ainv, P, rot, xyz, axes,
                             reorient34, *, eps=1e-8, with_img_path=True):
    """(g_rot (B,3), g_xyz (B,3)) of sum_b g_out[b] ncc[b]: ncc_backward, siddon_backward_pose and
    pose_euler_backward in one launch."""
    B, N = img.shape
    _blocked_record_only("siddon_ncc_backward_pose", aux, B, N)
    _fixed_rows("siddon_ncc_backward_pose", x1, B, N)
    shared = x1.shape[0] == 1 and B != 1
    g_out, g_stride = _batch_grad(g_out, B)
    x1, img, source, target = (t.contiguous() for t in (x1, img, source, target))
    held, chain = _pose_chain(Mw, Ainv, P, rot, xyz, axes, reorient34)
    dev = img.device
    g_rot, g_xyz = _pose_grads(B, dev)
    if B:
        _launch("ddrr_siddon_ncc_backward_pose", dev, aux.data_ptr(), img.data_ptr(), x1.data_ptr(),
                0 if shared else N, stats.data_ptr(), g_out.data_ptr(), g_stride, source.data_ptr(),
                target.data_ptr(), *chain, B, N, float(eps), int(bool(with_img_path)),
                siddon_ncc_workspace(B, dev).data_ptr(), g_rot.data_ptr(), g_xyz.data_ptr())
    return g_rot, g_xyz


def siddon_backward_pose_euler(aux, grad_out, source, Mw, Ainv, P, rot, xyz, axes, reorient34, *, eps=1e-8,
                               with_img_path=True):
    """(g_rot (B,3), g_xyz (B,3)) of any objective of the image with per-pixel gradient ``grad_out`` (B, N):
    siddon_backward_pose and pose_euler_backward in one launch (the rays as pose_raygen_forward made them)."""
    B, N = grad_out.shape
    _blocked_record_only("siddon_backward_pose_euler", aux, B, N)
    grad_out, source = grad_out.contiguous(), source.contiguous()
    held, chain = _pose_chain(Mw, Ainv, P, rot, xyz, axes, reorient34)
    dev = grad_out.device
    g_rot, g_xyz = _pose_grads(B, dev)
    if B:
        _launch("ddrr_siddon_backward_pose_euler", dev, aux.data_ptr(), grad_out.data_ptr(), source.data_ptr(),
                *chain, B, N, float(eps), int(bool(with_img_path)), siddon_ncc_workspace(B, dev).data_ptr(),
                g_rot.data_ptr(), g_xyz.data_ptr())
    return g_rot, g_xyz


def siddon_backward_volume(volume, source, target, img, grad_out, *, voxel_shift=0.5, eps=1e-8,
                           reducefn="sum", det=None, tile=None):
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    g_volume = torch.zeros_like(volume, memory_format=torch.contiguous_format)
    hints = _hints(det, tile, N)
    if _empty(B, N):
        return g_volume
    _launch(
        "ddrr_siddon_backward_volume", volume.device, *r.vol(volume), *r.rays(), r.ptr(grad_out), B, N,
        float(voxel_shift), float(eps), reduce_code(reducefn), *hints, g_volume.data_ptr())
    return g_volume


def siddon_backward_volume_bricks(volume_shape, source, target, img, grad_out, det, *,
                                  voxel_shift=0.5, eps=1e-8):
    """Detector-grid Siddon (sum) volume gradient through the volume-stationary brick
    kernel: every 32^3 brick of the gradient is accumulated in LDS and stored once.
    -> g_volume (Dx,Dy,Dz), fully written"""
    B, N, _ = target.shape
    H, W = _grid(det, N, source)
    _require_gpu(target)
    r = _Rays(source, target, img)
    Dx, Dy, Dz = (int(v) for v in volume_shape)
    g_volume = torch.empty(Dx, Dy, Dz, dtype=torch.float32, device=target.device)
    _launch("ddrr_siddon_backward_volume_bricks", target.device, Dx, Dy, Dz, *r.grid(), r.ptr(grad_out), B, H, W,
            float(voxel_shift), float(eps), g_volume.data_ptr(),
            launch_workspace((Dx, Dy, Dz), target.device).data_ptr())
    return g_volume


def siddon_forward_channels(volume, labels_u8, n_channels, source, target, img, *,
                            voxel_shift=0.5, eps=1e-8, det=None, tile=None):
    """-> (B, C, N)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    _check_labels(labels_u8, volume)
    out = torch.empty(B, n_channels, N, dtype=torch.float32, device=volume.device)
    hints = _hints(det, tile, N)
    if _empty(B, N):
        return out
    _launch(
        "ddrr_siddon_forward_channels", volume.device, r.ptr(volume), r.ptr(labels_u8), *volume.shape, *r.rays(),
        B, N, int(n_channels), float(voxel_shift), float(eps), *hints, out.data_ptr())
    return out


_words_cache = {}  # (id(volume), id(labels), C) -> _ChannelWords


class _ChannelWords:
    """Cache entry of :func:`channel_words`."""
    __slots__ = ("vol", "lab", "tracked", "words", "state", "seen", "churn")

    def __init__(self, vol, lab):
        self.vol, self.lab = vol, lab   # weak references
        self.tracked = None             # what PyTorch tracks of the pair when the words were last packed
        self.words = self.state = None
        self.seen = 0                   # renders of this pair in this tracked state
        self.churn = 0                  # repacks in a row because the pair had changed between two renders


def channel_words(volume, labels_u8, n_channels, build=True):
    """The channel render's staged words (value with a 16-bit mantissa | label) for the whole volume,
    one float per voxel, for a (volume, label map) pair that is rendered again and again:
    :func:`siddon_forward_channels_bricks` then stages a brick with straight 16-byte copies -- no label
    loads, no packing (one pose 0.089 -> 0.079 ms, 8 poses 0.280 -> 0.262 on the reference's example
    shape and label map, the comparison launches included).  Cached per (volume tensor, label tensor, channels) while both live;
    +100 % of the volume's bytes.  EVERY call launches ``ddrr_channel_words``: it compares a
    fingerprint of volume and labels on the device (1024 voxels each) and returns after a few
    microseconds if nothing changed; a change PyTorch tracks (version counters, storage addresses)
    forces the repack, one it does not (``volume.data[...] = x``) is found by the fingerprint.
    ``build=False``: None unless the pair has been seen before in its present state (the first render
    of a pair does not pay for a pass it may never use)."""
    key = (id(volume), id(labels_u8), int(n_channels))
    tracked = (volume._version, labels_u8._version, volume.data_ptr(), labels_u8.data_ptr())
    ent = _words_cache.get(key)
    if ent is None or ent.vol() is not volume or ent.lab() is not labels_u8:
        drop = lambda _, k=key: _words_cache.pop(k, None)  # noqa: E731
        ent = _words_cache[key] = _ChannelWords(weakref.ref(volume, drop), weakref.ref(labels_u8, drop))
    if not build:
        if ent.words is None:
            ent.seen = ent.seen + 1 if ent.tracked == tracked else 1
            ent.tracked = tracked
            if ent.seen < 2:
                return None
    force = ent.words is None or ent.tracked != tracked
    if not build:
        # a pair that changes between renders again and again (a volume edited in place every
        # iteration) gains nothing from words that are packed anew for every render: given up for it
        ent.churn = ent.churn + 1 if (force and ent.words is not None) else 0
        if ent.churn >= 3:
            ent.words = ent.state = None
            ent.tracked, ent.seen, ent.churn = tracked, -(1 << 30), 0
            return None
    if ent.words is None:
        ent.words = torch.empty_like(volume)
        n = int(_query("ddrr_channel_words_state_bytes"))
        ent.state = torch.zeros((n + 3) // 4, dtype=torch.int32, device=volume.device)
    ent.tracked = tracked
    if volume.numel():
        _launch("ddrr_channel_words", volume.device, volume.data_ptr(), labels_u8.data_ptr(), volume.numel(),
                int(n_channels), ent.words.data_ptr(), ent.state.data_ptr(), int(force))
    return ent.words


def channel_words_repacks(volume, labels_u8, n_channels):
    """How often the words of this pair were packed (1 after the first build; +1 for every change found
    by the tracked state or by the device-side fingerprint), or None.  Reads a word from the device."""
    ent = _words_cache.get((id(volume), id(labels_u8), int(n_channels)))
    if ent is None or ent.state is None or ent.vol() is not volume:
        return None
    return int(ent.state[1].item())


def siddon_forward_channels_bricks(volume, labels_u8, n_channels, source, target, img, det, *,
                                   voxel_shift=0.5, eps=1e-8, words=None):
    """:func:`siddon_forward_channels` for a detector grid on the volume-stationary brick
    kernel (the label rides in the low byte of the staged voxel word).  ``words``: the volume's
    ready-packed words (:func:`channel_words`) -- staged as they are.  -> (B, C, N)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    H, W = _grid(det, N, source)
    _check_labels(labels_u8, volume)
    out = torch.empty(B, n_channels, N, dtype=torch.float32, device=volume.device)
    if _empty(B, N):
        return out
    if words is not None:
        if words.shape != volume.shape or words.dtype != torch.float32 or not words.is_contiguous():
            raise ValueError("words: channel_words(volume, labels, n_channels)")
        _launch("ddrr_siddon_forward_channels_bricks_words", volume.device, words.data_ptr(), *volume.shape,
                *r.grid(), B, H, W, int(n_channels), float(voxel_shift), float(eps), out.data_ptr(),
                launch_workspace(volume.shape, volume.device).data_ptr())
        return out
    _launch("ddrr_siddon_forward_channels_bricks", volume.device, r.ptr(volume), r.ptr(labels_u8), *volume.shape,
            *r.grid(), B, H, W, int(n_channels), float(voxel_shift), float(eps), out.data_ptr(),
            launch_workspace(volume.shape, volume.device).data_ptr())
    return out


def siddon_backward_channels_bricks(volume, labels_u8, source, target, img, grad_out, det, *,
                                    voxel_shift=0.5, eps=1e-8, want_img=True):
    """Ray / img gradients of :func:`siddon_forward_channels_bricks` for grad_out (B, C, N) on the
    volume-stationary bricks: the brick kernel writes the backward record of the volume weighted by
    every voxel's own incoming gradient, ``ddrr_siddon_backward_rays`` turns it into gradients.
    -> (g_source per ray (B,N,3), g_target (B,N,3), g_img (B,N) | None)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    C = _channels(grad_out, B, N)
    H, W = _grid(det, N, source)
    dev = volume.device
    aux = brick_record_buffer(B, N, dev)
    ones = torch.ones(B, N, dtype=torch.float32, device=dev)
    if not _empty(B, N):
        _launch("ddrr_siddon_backward_channels_bricks", dev, r.ptr(volume), r.ptr(labels_u8), *volume.shape,
                r.source.data_ptr(), r.target.data_ptr(), r.ptr(grad_out), B, H, W, int(C), float(voxel_shift),
                float(eps), aux.data_ptr(), launch_workspace(volume.shape, dev).data_ptr())
    return siddon_backward_rays(aux, ones, r.source, r.target, r.img, eps=eps, want_img_grad=want_img)


def siddon_backward_channels_volume_bricks(labels_u8, source, target, img, grad_out, det, *,
                                           voxel_shift=0.5, eps=1e-8):
    """Volume gradient of :func:`siddon_forward_channels_bricks` for grad_out (B, C, N) on the
    volume-stationary bricks (the LDS brick is the accumulator, the voxel's label rides in the
    word's low byte).  -> g_volume, the label map's shape"""
    B, N, _ = target.shape
    C = _channels(grad_out, B, N)
    H, W = _grid(det, N, source)
    _check_labels(labels_u8)
    _require_gpu(target)
    dev = target.device
    r = _Rays(source, target, img)
    g_volume = torch.empty(labels_u8.shape, dtype=torch.float32, device=dev)
    _launch("ddrr_siddon_backward_channels_volume_bricks", dev, *r.vol(labels_u8), *r.grid(), r.ptr(grad_out), B,
            H, W, int(C), float(voxel_shift), float(eps), g_volume.data_ptr(),
            launch_workspace(labels_u8.shape, dev).data_ptr())
    return g_volume


def channels_fit_bricks(B, C, N):
    """One brick launch addresses the (B, C, N) result with 32-bit byte offsets."""
    return B * C * N < 2 ** 30 and N < 2 ** 22


def siddon_backward_midpoint(volume, source, target, img, grad_out, *, voxel_shift=0.5, eps=1e-8,
                             lookup="mid_nearest", align_corners=False, want_rays=True,
                             want_img=True, want_volume=False):
    """Backward of :func:`siddon_forward` for the midpoint lookups (reduce sum).
    -> (g_source per ray, g_target, g_img, g_volume), None where not asked."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    g = _grad_buffers(B, N, torch.float32, volume.device, rays=want_rays, img=want_img,
                      volume_shape=volume.shape if want_volume else None)
    if not _empty(B, N):
        _launch("ddrr_siddon_backward_midpoint", volume.device, *r.vol(volume), *r.rays(), r.ptr(grad_out), B, N,
                float(voxel_shift), float(eps), _LOOKUP[lookup], int(bool(align_corners)), *map(_ptr, g.values()))
    return tuple(g.values())


def siddon_segments(volume, source, target, img, *, voxel_shift=0.5, eps=1e-8):
    """The per-segment terms a callable ``reducefn`` receives (renderers.py:70-71).
    -> (B, M-1, N) with M = Dx+Dy+Dz+3; transpose(1, 2) is the reference's layout."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    M1 = sum(int(v) for v in volume.shape) + 2
    terms = torch.empty(B, M1, N, dtype=torch.float32, device=volume.device)
    if not _empty(B, N):
        _launch("ddrr_siddon_segments", volume.device, *r.vol(volume), *r.rays(), B, N, float(voxel_shift),
                float(eps), terms.data_ptr())
    return terms


def siddon_segments_backward(volume, source, target, img, grad_terms, *, voxel_shift=0.5, eps=1e-8,
                             want_rays=True, want_img=True, want_volume=False):
    """Backward of :func:`siddon_segments` for grad_terms (B, M-1, N).
    -> (g_source per ray, g_target, g_img, g_volume), None where not asked."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    g = _grad_buffers(B, N, torch.float32, volume.device, rays=want_rays, img=want_img,
                      volume_shape=volume.shape if want_volume else None)
    if not _empty(B, N):
        _launch("ddrr_siddon_segments_backward", volume.device, *r.vol(volume), *r.rays(), r.ptr(grad_terms), B, N,
                float(voxel_shift), float(eps), *map(_ptr, g.values()))
    return tuple(g.values())


def siddon_backward_channels(volume, labels_u8, source, target, img, grad_out, *, voxel_shift=0.5,
                             eps=1e-8, want_rays=True, want_img=True, want_volume=False,
                             det=None, tile=None):
    """Backward of :func:`siddon_forward_channels` for grad_out (B, C, N).
    -> (g_source per ray (B,N,3), g_target (B,N,3), g_img (B,N), g_volume), None where not asked."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    C = _channels(grad_out, B, N)
    g = _grad_buffers(B, N, torch.float32, volume.device, rays=want_rays, img=want_img,
                      volume_shape=volume.shape if want_volume else None)
    hints = _hints(det, tile, N)
    if not _empty(B, N):
        _launch(
            "ddrr_siddon_backward_channels", volume.device, r.ptr(volume), r.ptr(labels_u8), *volume.shape,
            *r.rays(), r.ptr(grad_out), B, N, int(C), float(voxel_shift), float(eps), *hints,
            *map(_ptr, g.values()))
    return tuple(g.values())


def trilinear_alpha_range(source, target, volume_shape, *, voxel_shift=0.5, eps=1e-8):
    """The batch-global marching range of reference renderers.py:220-223 in one pass over the
    rays (no gradient flows through it).  -> (alphamin, alphamax), 0-dim device tensors."""
    _require_gpu(target)
    B, N, _ = target.shape
    if source.dtype != torch.float32 or target.dtype != torch.float32:
        raise NotImplementedError("trilinear_alpha_range needs float32 rays")
    source, target = source.contiguous(), target.contiguous()
    rng = torch.empty(2, dtype=torch.float32, device=target.device)
    _launch("ddrr_trilinear_alpha_range", target.device, source.data_ptr(), source.shape[1],
            target.data_ptr(), B, N, *(int(v) for v in volume_shape), float(voxel_shift),
            float(eps), rng.data_ptr())
    return rng[0], rng[1]


def trilinear_forward(volume, source, target, img, alphamin, alphamax, *, n_points=500,
                      voxel_shift=0.5, eps=1e-8, reducefn="sum", mode="bilinear",
                      align_corners=False, det=None, tile=None):
    """alphamin / alphamax: 0-dim (or 1-element) device tensors.  -> out (B,N)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    out = torch.empty(B, N, dtype=torch.float32, device=volume.device)
    hints = _hints(det, tile, N)
    if _empty(B, N):
        return out
    _launch(
        "ddrr_trilinear_forward", volume.device, *r.vol(volume), *r.rays(), B, N, float(voxel_shift), float(eps),
        int(n_points), alphamin.data_ptr(), alphamax.data_ptr(), int(mode == "nearest"),
        reduce_code(reducefn), int(bool(align_corners)), *hints, out.data_ptr())
    return out


def trilinear_forward_channels(volume, labels_u8, n_channels, source, target, img, alphamin,
                               alphamax, *, n_points=500, voxel_shift=0.5, eps=1e-8,
                               align_corners=False, det=None, tile=None):
    """Trilinear.forward with a mask (renderers.py:242-252).  -> (B, C, N)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    _check_labels(labels_u8, volume)
    out = torch.empty(B, n_channels, N, dtype=torch.float32, device=volume.device)
    hints = _hints(det, tile, N)
    if _empty(B, N):
        return out
    _launch(
        "ddrr_trilinear_forward_channels", volume.device, r.ptr(volume), r.ptr(labels_u8), *volume.shape,
        *r.rays(), B, N, int(n_channels), float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(),
        alphamax.data_ptr(), int(bool(align_corners)), *hints, out.data_ptr())
    return out


def trilinear_forward_channels_bricks(volume, labels_u8, n_channels, source, target, img,
                                      alphamin, alphamax, det, *, n_points=500, voxel_shift=0.5,
                                      eps=1e-8):
    """The marcher's mask_to_channels for a detector grid on the volume-stationary bricks
    (ddrr_trilinear_forward_channels_bricks; mode "bilinear", align_corners=False).  -> (B, C, N)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    H, W = _grid(det, N, source)
    _check_labels(labels_u8, volume)
    out = torch.empty(B, n_channels, N, dtype=torch.float32, device=volume.device)
    if _empty(B, N):
        return out
    _launch(
        "ddrr_trilinear_forward_channels_bricks", volume.device, r.ptr(volume), r.ptr(labels_u8), *volume.shape,
        *r.grid(), B, H, W, int(n_channels), float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(),
        alphamax.data_ptr(), out.data_ptr(), launch_workspace(volume.shape, volume.device).data_ptr())
    return out


def trilinear_backward_channels_volume_bricks(labels_u8, source, target, img, grad_out, alphamin,
                                              alphamax, det, *, n_points=500, voxel_shift=0.5,
                                              eps=1e-8):
    """Volume gradient of :func:`trilinear_forward_channels_bricks` for grad_out (B, C, N) on the
    owner bricks (LDS accumulator, labels in the words' low byte).  -> g_volume, the label map's
    shape"""
    B, N, _ = target.shape
    C = _channels(grad_out, B, N)
    H, W = _grid(det, N, source)
    _check_labels(labels_u8)
    _require_gpu(target)
    dev = target.device
    r = _Rays(source, target, img)
    g_volume = torch.empty(labels_u8.shape, dtype=torch.float32, device=dev)
    _launch("ddrr_trilinear_backward_channels_volume_bricks", dev, *r.vol(labels_u8), *r.grid(), r.ptr(grad_out),
            B, H, W, int(C), float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(),
            alphamax.data_ptr(), g_volume.data_ptr(), launch_workspace(labels_u8.shape, dev).data_ptr())
    return g_volume


def trilinear_backward_channels_bricks(volume, labels_u8, source, target, img, grad_out, alphamin,
                                       alphamax, det, *, n_points=500, voxel_shift=0.5, eps=1e-8,
                                       want_rays=True, want_img=True, want_alpha=True):
    """Ray / img / range gradients of :func:`trilinear_forward_channels_bricks` for grad_out
    (B, C, N) on the volume-stationary bricks: the brick kernel writes the marcher's record with
    every sample weighted by the incoming gradient of its channel,
    ``ddrr_trilinear_backward_rays`` turns it into gradients.  Results as
    :func:`trilinear_backward` (without g_volume)."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    C = _channels(grad_out, B, N)
    H, W = _grid(det, N, source)
    dev = volume.device
    aux = torch.empty(TRI_AUX_PLANES, B, N, dtype=torch.float32, device=dev)
    ones = torch.ones(B, N, dtype=torch.float32, device=dev)
    if not _empty(B, N):
        _launch("ddrr_trilinear_backward_channels_bricks", dev, r.ptr(volume), r.ptr(labels_u8), *volume.shape,
                r.source.data_ptr(), r.target.data_ptr(), r.ptr(grad_out), B, H, W, int(C), float(voxel_shift),
                float(eps), int(n_points), alphamin.data_ptr(), alphamax.data_ptr(), aux.data_ptr(),
                launch_workspace(volume.shape, dev).data_ptr())
    return trilinear_backward_rays(aux, ones, r.source, r.target, r.img, alphamin, alphamax,
                                   n_points=n_points, eps=eps, want_rays=want_rays,
                                   want_img=want_img, want_alpha=want_alpha)


def trilinear_forward_bricks(volume, source, target, img, alphamin, alphamax, det, *,
                             n_points=500, voxel_shift=0.5, eps=1e-8, want_aux=False):
    """Detector-grid trilinear march (bilinear, sum, align_corners=False) through the
    volume-stationary brick kernel.  -> out (B,N), or (out, aux (7,B,N)) with ``want_aux``:
    the planar backward record for :func:`trilinear_backward_rays`."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    H, W = _grid(det, N, source)
    out = torch.empty(B, N, dtype=torch.float32, device=volume.device)
    aux = torch.empty(TRI_AUX_PLANES, B, N, dtype=torch.float32, device=volume.device) \
        if want_aux else None
    if not _empty(B, N):
        _launch("ddrr_trilinear_forward_bricks", volume.device, *r.vol(volume), *r.grid(), B, H, W,
                float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(), alphamax.data_ptr(),
                out.data_ptr(), _ptr(aux), launch_workspace(volume.shape, volume.device).data_ptr())
    return (out, aux) if want_aux else out


def trilinear_backward_rays(aux, grad_out, source, target, img, alphamin, alphamax, *,
                            n_points=500, eps=1e-8, want_rays=True, want_img=True,
                            want_alpha=True):
    """Ray / range gradients of the march from the record of :func:`trilinear_forward_bricks`;
    results as :func:`trilinear_backward` (without g_volume)."""
    B, N, _ = target.shape
    _require_gpu(target)
    res = _grad_buffers(B, N, torch.float32, target.device, rays=want_rays, img=want_img, alpha=want_alpha)
    if not _empty(B, N):
        r = _Rays(source, target, img)
        _launch("ddrr_trilinear_backward_rays", target.device, aux.data_ptr(), r.ptr(grad_out), *r.grid(), B, N,
                float(eps), int(n_points), alphamin.data_ptr(), alphamax.data_ptr(),
                *(_ptr(res[k]) for k in ("g_source", "g_target", "g_img", "g_alpha")))
    return res


def trilinear_backward_volume_bricks(volume_shape, source, target, img, grad_out, alphamin,
                                     alphamax, det, *, n_points=500, voxel_shift=0.5, eps=1e-8):
    """Volume gradient of the detector-grid trilinear march through the brick kernel (LDS
    accumulation).  -> g_volume (Dx,Dy,Dz)"""
    B, N, _ = target.shape
    H, W = _grid(det, N, source)
    _require_gpu(target)
    r = _Rays(source, target, img)
    Dx, Dy, Dz = (int(v) for v in volume_shape)
    g_volume = torch.empty(Dx, Dy, Dz, dtype=torch.float32, device=target.device)
    _launch("ddrr_trilinear_backward_volume_bricks", target.device, Dx, Dy, Dz, *r.grid(), r.ptr(grad_out), B, H,
            W, float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(),
            alphamax.data_ptr(), g_volume.data_ptr(),
            launch_workspace((Dx, Dy, Dz), target.device).data_ptr())
    return g_volume


def trilinear_samples(volume, source, target, img, alphamin, alphamax, *, n_points=500,
                      voxel_shift=0.5, eps=1e-8, mode="bilinear", align_corners=False):
    """The per-sample terms a callable ``reducefn`` of the marcher receives
    (renderers.py:226-238).  -> (B, P, N); transpose(1, 2) is the reference's layout."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    out = torch.empty(B, int(n_points), N, dtype=torch.float32, device=volume.device)
    if not _empty(B, N):
        _launch("ddrr_trilinear_samples", volume.device, *r.vol(volume), *r.rays(), B, N, float(voxel_shift),
                float(eps), int(n_points), alphamin.data_ptr(), alphamax.data_ptr(), int(mode == "nearest"),
                int(bool(align_corners)), out.data_ptr())
    return out


def trilinear_samples_backward(volume, source, target, img, grad_samples, alphamin, alphamax, *,
                               n_points=500, voxel_shift=0.5, eps=1e-8, mode="bilinear",
                               align_corners=False, want_rays=True, want_img=True,
                               want_alpha=True, want_volume=False):
    """Backward of :func:`trilinear_samples` for grad_samples (B, P, N); results as
    :func:`trilinear_backward`."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    res = _grad_buffers(B, N, torch.float32, volume.device, rays=want_rays, img=want_img, alpha=want_alpha,
                        volume_shape=volume.shape if want_volume else None)
    if not _empty(B, N):
        _launch("ddrr_trilinear_samples_backward", volume.device, *r.vol(volume), *r.rays(), r.ptr(grad_samples),
                B, N, float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(), alphamax.data_ptr(),
                int(mode == "nearest"), int(bool(align_corners)), *map(_ptr, res.values()))
    return res


def trilinear_backward_channels(volume, labels_u8, source, target, img, grad_out, alphamin,
                                alphamax, *, n_points=500, voxel_shift=0.5, eps=1e-8,
                                align_corners=False, want_rays=True, want_img=True,
                                want_alpha=True, want_volume=False, det=None, tile=None):
    """Backward of :func:`trilinear_forward_channels` for grad_out (B, C, N); results as
    :func:`trilinear_backward`."""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    C = _channels(grad_out, B, N)
    res = _grad_buffers(B, N, torch.float32, volume.device, rays=want_rays, img=want_img, alpha=want_alpha,
                        volume_shape=volume.shape if want_volume else None)
    hints = _hints(det, tile, N)
    if not _empty(B, N):
        _launch(
            "ddrr_trilinear_backward_channels", volume.device, r.ptr(volume), r.ptr(labels_u8), *volume.shape,
            *r.rays(), r.ptr(grad_out), B, N, int(C), float(voxel_shift), float(eps), int(n_points),
            alphamin.data_ptr(), alphamax.data_ptr(), int(bool(align_corners)), *hints, *map(_ptr, res.values()))
    return res


def trilinear_backward(volume, source, target, img, grad_out, alphamin, alphamax, *, n_points=500,
                       voxel_shift=0.5, eps=1e-8, mode="bilinear", align_corners=False,
                       want_rays=True, want_img=True, want_alpha=True, want_volume=False,
                       det=None, tile=None, reducefn="sum"):
    """-> dict(g_source per ray, g_target, g_img, g_alpha (B,N,2), g_volume)"""
    r = _rays(volume, source, target, img)
    B, N = r.B, r.N
    res = _grad_buffers(B, N, torch.float32, volume.device, rays=want_rays, img=want_img, alpha=want_alpha,
                        volume_shape=volume.shape if want_volume else None)
    hints = _hints(det, tile, N)
    if _empty(B, N):
        return res
    # (reduce "max" has no tiled form: no detector hints)
    maxed = reduce_code(reducefn) == REDUCE_MAX
    _launch(
        "ddrr_trilinear_backward_max" if maxed else "ddrr_trilinear_backward", volume.device, *r.vol(volume),
        *r.rays(), r.ptr(grad_out), B, N, float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(),
        alphamax.data_ptr(), int(mode == "nearest"), int(bool(align_corners)), *(() if maxed else hints),
        *map(_ptr, res.values()))
    return res


# ---------------------------------------------------------------- double precision
# (`DRR(...).to(torch.float64)`, reference drr.py:71-75: per-ray kernels of csrc/f64_rays.hip)

def siddon_forward_f64(volume, source, target, img, *, voxel_shift=0.5, eps=1e-8, reducefn="sum",
                       want_aux=False):
    """-> (out (B,N) float64, aux (B,N,8) float64 | None)"""
    r = _rays(volume, source, target, img, torch.float64)
    B, N = r.B, r.N
    out = torch.empty(B, N, dtype=torch.float64, device=volume.device)
    aux = torch.empty(B, N, SIDDON_AUX, dtype=torch.float64, device=volume.device) \
        if want_aux else None
    if not _empty(B, N):
        _launch("ddrr_siddon_forward_f64", volume.device, *r.vol(volume), *r.rays(), B, N, float(voxel_shift),
                float(eps), reduce_code(reducefn), out.data_ptr(), _ptr(aux))
    return out, aux


def siddon_backward_f64(volume_shape, source, target, img, grad_out, aux, *, voxel_shift=0.5,
                        eps=1e-8, want_rays=True, want_img=True, want_volume=False):
    """-> (g_source per ray (B,N,3), g_target (B,N,3), g_img (B,N), g_volume), None where not asked"""
    B, N, _ = target.shape
    dims = tuple(int(v) for v in volume_shape)
    g = _grad_buffers(B, N, torch.float64, target.device, rays=want_rays, img=want_img,
                      volume_shape=dims if want_volume else None)
    if not _empty(B, N):
        r = _Rays(source, target, img)
        _launch("ddrr_siddon_backward_f64", target.device, *dims, *r.rays(), r.ptr(grad_out), _ptr(aux), B, N,
                float(voxel_shift), float(eps), *map(_ptr, g.values()))
    return tuple(g.values())


def trilinear_forward_f64(volume, source, target, img, alphamin, alphamax, *, n_points=500,
                          voxel_shift=0.5, eps=1e-8):
    r = _rays(volume, source, target, img, torch.float64)
    B, N = r.B, r.N
    out = torch.empty(B, N, dtype=torch.float64, device=volume.device)
    if not _empty(B, N):
        _launch("ddrr_trilinear_forward_f64", volume.device, *r.vol(volume), *r.rays(), B, N, float(voxel_shift),
                float(eps), int(n_points), alphamin.data_ptr(), alphamax.data_ptr(), out.data_ptr())
    return out


def trilinear_backward_f64(volume, source, target, img, grad_out, alphamin, alphamax, *,
                           n_points=500, voxel_shift=0.5, eps=1e-8, want_rays=True, want_img=True,
                           want_alpha=True, want_volume=False):
    """-> dict(g_source per ray, g_target, g_img, g_alpha (B,N,2), g_volume)"""
    r = _rays(volume, source, target, img, torch.float64)
    B, N = r.B, r.N
    res = _grad_buffers(B, N, torch.float64, volume.device, rays=want_rays, img=want_img, alpha=want_alpha,
                        volume_shape=volume.shape if want_volume else None)
    if not _empty(B, N):
        _launch("ddrr_trilinear_backward_f64", volume.device, *r.vol(volume), *r.rays(), r.ptr(grad_out), B, N,
                float(voxel_shift), float(eps), int(n_points), alphamin.data_ptr(), alphamax.data_ptr(),
                *map(_ptr, res.values()))
    return res


# ---------------------------------------------------------------- the materialising general path
# (csrc/general_rays.hip: the per-segment / per-sample tensors of the reference and their
# autograd, float32 or float64, for the keyword combinations the fused kernels do not take)

def _general_rays(volume, source, target, img):
    """-> (the checked batch, the f64 flag): the general path renders in the volume's dtype."""
    if volume.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"the general path renders float32 or float64, not {volume.dtype}")
    return _rays(volume, source, target, img, volume.dtype), int(volume.dtype == torch.float64)


def siddon_segments_general(volume, source, target, img, *, voxel_shift=0.5, eps=1e-8,
                            lookup="step", align_corners=False, raw=False):
    """-> terms (B, M-1, N), M = Dx+Dy+Dz+3: ``img * value * interval`` per segment
    (renderers.py:66-71), or with ``raw`` the looked-up values alone (the label lookup)."""
    r, f64 = _general_rays(volume, source, target, img)
    B, N = r.B, r.N
    M1 = sum(volume.shape) + 2
    terms = torch.empty(B, M1, N, dtype=volume.dtype, device=volume.device)
    if not _empty(B, N):
        _launch("ddrr_siddon_segments_general", volume.device, r.ptr(volume), f64, *volume.shape, *r.rays(), B, N,
                float(voxel_shift), float(eps), _LOOKUP[lookup], int(bool(align_corners)), int(bool(raw)),
                terms.data_ptr())
    return terms


def siddon_segments_general_backward(volume, source, target, img, grad_terms, *, voxel_shift=0.5,
                                     eps=1e-8, lookup="step", align_corners=False,
                                     through_lookup=True, want_rays=True, want_img=True,
                                     want_volume=False):
    """-> (g_source per ray (B,N,3), g_target (B,N,3), g_img (B,N), g_volume), None where not asked"""
    r, f64 = _general_rays(volume, source, target, img)
    B, N = r.B, r.N
    g = _grad_buffers(B, N, volume.dtype, volume.device, rays=want_rays, img=want_img and through_lookup,
                      volume_shape=volume.shape if want_volume and through_lookup else None)
    if not _empty(B, N):
        _launch("ddrr_siddon_segments_general_backward", volume.device, r.ptr(volume), f64, *volume.shape,
                *r.rays(), r.ptr(grad_terms.to(volume.dtype)), B, N, float(voxel_shift), float(eps),
                _LOOKUP[lookup], int(bool(align_corners)), int(bool(through_lookup)), *map(_ptr, g.values()))
    elif g["g_img"] is not None:
        g["g_img"].zero_()
    return tuple(g.values())


def trilinear_samples_general(volume, source, target, img, alphamin, alphamax, *, n_points=500,
                              voxel_shift=0.5, eps=1e-8, mode="bilinear", align_corners=False,
                              raw=False):
    """-> samples (B, P, N): ``img * step * value`` per sample (renderers.py:224-236), or with
    ``raw`` the looked-up values alone (the label lookup)."""
    r, f64 = _general_rays(volume, source, target, img)
    B, N = r.B, r.N
    samples = torch.empty(B, int(n_points), N, dtype=volume.dtype, device=volume.device)
    if not _empty(B, N):
        _launch("ddrr_trilinear_samples_general", volume.device, r.ptr(volume), f64, *volume.shape, *r.rays(), B,
                N, float(voxel_shift), float(eps), int(n_points), r.ptr(alphamin.to(volume.dtype).reshape(1)),
                r.ptr(alphamax.to(volume.dtype).reshape(1)), int(mode == "nearest"), int(bool(align_corners)),
                int(bool(raw)), samples.data_ptr())
    return samples


def trilinear_samples_general_backward(volume, source, target, img, grad_samples, alphamin,
                                       alphamax, *, n_points=500, voxel_shift=0.5, eps=1e-8,
                                       mode="bilinear", align_corners=False, want_rays=True,
                                       want_img=True, want_alpha=True, want_volume=False):
    """-> dict(g_source per ray, g_target, g_img, g_alpha (B,N,2) per ray, g_volume)"""
    r, f64 = _general_rays(volume, source, target, img)
    B, N = r.B, r.N
    res = _grad_buffers(B, N, volume.dtype, volume.device, rays=want_rays, img=want_img, alpha=want_alpha,
                        volume_shape=volume.shape if want_volume else None, new=torch.zeros)
    if not _empty(B, N):
        _launch("ddrr_trilinear_samples_general_backward", volume.device, r.ptr(volume), f64, *volume.shape,
                *r.rays(), r.ptr(grad_samples.to(volume.dtype)), B, N, float(voxel_shift), float(eps),
                int(n_points), r.ptr(alphamin.to(volume.dtype).reshape(1)),
                r.ptr(alphamax.to(volume.dtype).reshape(1)), int(mode == "nearest"), int(bool(align_corners)),
                *map(_ptr, res.values()))
    return res


# ------------------------------------------------------------------ MutualInformation (libdiffdrr_mi_hip.so)
def _mi_image(x, B, N):
    """(B or 1, H, W) -> (tensor, stride in floats): ONE image shared by the batch (an expanded tensor or
    a single image) is read in place with stride 0."""
    if x.shape[0] == 1 and B != 1 or (B > 1 and x.stride(0) == 0):
        return x[:1].contiguous(), 0
    return x.contiguous(), N


def _launch_wmi(name, device, *args):
    """:func:`_launch` through the weighted MutualInformation library (libdiffdrr_wmi_hip.so)."""
    _launch_on(_lib.get_wmi_lib(), name, device, args)


def _query_wmi(name, *args):
    # (not called here: the seam tests/test_wmi_abi.py uses to see a missing library fail loudly)
    return _lib.get_wmi_lib().query(name, *args)


def _wmi_weight(name, w, B, H, W):
    """(B or 1, H, W) float32 -> (tensor, stride in floats): ONE weight shared by the batch (given so, or
    `expand`ed) is read in place with stride 0."""
    if w.dim() != 3 or tuple(w.shape[1:]) != (H, W) or w.shape[0] not in (1, B) or w.dtype != torch.float32:
        raise ValueError(f"{name}: the weight has shape {tuple(w.shape)} {w.dtype}: float32 ({B}, {H}, {W}), or "
                         f"(1, {H}, {W}) for one weight shared by the batch, expected")
    return _mi_image(w, B, H * W)


def _mi_library(w):
    """(entry prefix, library, launcher) that serve a call without / with a weight"""
    if w is None:
        lib = _lib.get_mi_lib()
        return "ddrr_mi", lib, lambda name, device, *args: _launch_on(lib, name, device, args)
    return "ddrr_wmi", _lib.get_wmi_lib(), _launch_wmi


def _mi_forward(x1, x2, w, bins, sigma, epsilon, normalize, B, want_state, want_weight_sum=False):
    """:func:`mi_forward` (w None) and :func:`wmi_forward` -> (mi, state | None, weight_sum | None); the weighted
    entry takes the weight and its stride after the images and `weight_sum` after `state`."""
    _require_gpu(x2)
    for x in (x1, x2):
        if x.shape[0] not in (1, B):
            raise ValueError(f"image batch {x.shape[0]} is neither 1 nor B = {B}")
    H, W = x2.shape[-2:]
    K = bins.numel()
    wt, sw = (None, None) if w is None else _wmi_weight("wmi_forward", w, B, H, W)
    wargs = () if w is None else (wt.data_ptr(), sw)
    prefix, lib, launch = _mi_library(w)
    a, s1 = _mi_image(x1, B, H * W)
    b, s2 = _mi_image(x2, B, H * W)
    bins, sigma = bins.contiguous(), sigma.contiguous()
    dev = x2.device
    out = torch.empty(B, dtype=torch.float32, device=dev)
    state = None
    if want_state:
        state = torch.empty(B, int(lib.query(prefix + "_state_floats", K)), dtype=torch.float32, device=dev)
    weight_sum = torch.empty(B, dtype=torch.float64, device=dev) if want_weight_sum else None
    if B:
        n = int(lib.query(prefix + "_workspace_bytes", B, H, W, K))
        if n < 0:
            raise ValueError(lib._last_error().decode(errors="replace"))
        ws = torch.empty((n + 15) // 16, 4, dtype=torch.float32, device=dev)  # (16-byte aligned)
        launch(prefix + "_forward", dev, a.data_ptr(), s1, b.data_ptr(), s2, *wargs, B, H, W, bins.data_ptr(), K,
               sigma.data_ptr(), float(epsilon), int(bool(normalize)), ws.data_ptr(), ws.numel() * 4, out.data_ptr(),
               _ptr(state), *(() if w is None else (_ptr(weight_sum),)))
    return out, state, weight_sum


def _mi_backward(x1, x2, w, bins, sigma, state, g_out, which, B):
    """:func:`mi_backward` (w None) and :func:`wmi_backward`"""
    H, W = x2.shape[-2:]
    wt, sw = (None, None) if w is None else _wmi_weight("wmi_backward", w, B, H, W)
    wargs = () if w is None else (wt.data_ptr(), sw)
    prefix, _, launch = _mi_library(w)
    a, s1 = _mi_image(x1, B, H * W)
    b, s2 = _mi_image(x2, B, H * W)
    g_out, g_stride = _batch_grad(g_out, B)
    grad = torch.empty(B, H, W, dtype=torch.float32, device=x2.device)
    if B:
        launch(prefix + "_backward", x2.device, a.data_ptr(), s1, b.data_ptr(), s2, *wargs, B, H, W, bins.data_ptr(),
               bins.numel(), sigma.data_ptr(), state.data_ptr(), int(which), g_out.data_ptr(), g_stride,
               grad.data_ptr())
    return grad


def mi_forward(x1, x2, bins, sigma, epsilon, normalize, B, want_state=True):
    """MutualInformation (reference metrics.py:110-139) of B image pairs: x1, x2 (B or 1, H, W) fp32 on the
    device (either or both may be ONE image shared by the batch: the batch size is B, not derived from the
    shapes); bins (K,), sigma (0-dim): the module's buffers, read on the device.
    -> (mi (B), state (B, S) | None: what :func:`mi_backward` needs)."""
    return _mi_forward(x1, x2, None, bins, sigma, epsilon, normalize, B, want_state)[:2]


def mi_backward(x1, x2, bins, sigma, state, g_out, which, B):
    """g_out[b] * d mi[b] / d x2[b] (which = 1) or / d x1[b] (which = 0), (B, H, W), of :func:`mi_forward`
    with the same arguments.  A shared differentiated image gets its per-pose gradients (B, H, W)."""
    return _mi_backward(x1, x2, None, bins, sigma, state, g_out, which, B)


# ------------------------------------------------------------------ weighted MutualInformation (libdiffdrr_wmi_hip.so)
def wmi_forward(x1, x2, w, bins, sigma, epsilon, normalize, B, want_state=True, want_weight_sum=False):
    """:func:`mi_forward` under per-pixel weights w (B or 1, H, W) float32, >= 0 and finite (not looked for;
    include/diffdrr_wmi_hip.h): pixels with w == 0 are not read, a pair whose weights are all 0 scores 0.
    -> (mi (B), state (B, S) | None: what :func:`wmi_backward` needs[, the pairs' sums of weights (B) float64,
    with ``want_weight_sum``])."""
    res = _mi_forward(x1, x2, w, bins, sigma, epsilon, normalize, B, want_state, want_weight_sum)
    return res if want_weight_sum else res[:2]


def wmi_backward(x1, x2, w, bins, sigma, state, g_out, which, B):
    """g_out[b] * d mi[b] / d x2[b] (which = 1) or / d x1[b] (which = 0), (B, H, W), of :func:`wmi_forward`
    with the same arguments; exactly 0 where w == 0.  A shared differentiated image gets its per-pose gradients
    (B, H, W)."""
    return _mi_backward(x1, x2, w, bins, sigma, state, g_out, which, B)


# ------------------------------------------------------------------ reconstruction (libdiffdrr_recon_hip.so)
_TV_MODES = {"isotropic": _lib.RECON_TV_ISOTROPIC, "anisotropic": _lib.RECON_TV_ANISOTROPIC}


def _check_volume_like(name, t, like=None):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous float32 tensor expected")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{name}: shape {tuple(t.shape)} on {t.device}, expected {tuple(like.shape)} on {like.device}")


def tv3d(volume, spacing=(1.0, 1.0, 1.0), mode="isotropic", eps=1e-3, grad=None, accumulate=False, weight=1.0,
         scale=None):
    """3-D total variation of `volume` (Dx, Dy, Dz) fp32 on the device, and its gradient in the same pass
    (include/diffdrr_recon_hip.h ddrr_recon_tv3d): `grad` None -> the value only; else `grad` (same shape)
    = w dTV/dV, or += w dTV/dV with `accumulate`, where w = weight * scale (`scale`: a 1-element device
    tensor or None, read on the device).  -> the unweighted value, a 0-dim device tensor."""
    if not torch.is_tensor(volume) or volume.dim() != 3:
        raise ValueError("tv3d: a (Dx, Dy, Dz) volume expected")
    _check_volume_like("tv3d: volume", volume)
    _require_gpu(volume)
    if mode not in _TV_MODES:
        raise ValueError(f"tv3d: mode must be 'isotropic' or 'anisotropic', not {mode!r}")
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3 or not all(0.0 < s < float("inf") for s in spacing):
        raise ValueError(f"tv3d: spacing must be three positive numbers, not {spacing}")
    if not 0.0 <= float(eps) < float("inf"):
        raise ValueError(f"tv3d: eps must be >= 0, not {eps}")
    if max(volume.shape) > _lib.RECON_MAX_DIM or volume.numel() > 2**34:
        raise ValueError(f"tv3d: at most {_lib.RECON_MAX_DIM} voxels per axis and 2^34 in all, got {tuple(volume.shape)}")
    if grad is not None:
        _check_volume_like("tv3d: grad", grad, volume)
    elif accumulate:
        raise ValueError("tv3d: accumulate needs a grad tensor")
    if scale is not None:
        if (not torch.is_tensor(scale) or scale.dtype != torch.float32 or scale.numel() != 1
                or scale.device != volume.device):
            raise ValueError("tv3d: scale must be a 1-element float32 tensor on the volume's device")
    dev = volume.device
    if volume.numel() == 0:
        return torch.zeros((), dtype=torch.float32, device=dev)
    lib = _lib.get_recon_lib()
    dims = tuple(int(d) for d in volume.shape)
    n = int(lib.query("ddrr_recon_tv_workspace_bytes", *dims))
    if n < 0:
        raise ValueError(lib._last_error().decode(errors="replace"))
    ws = torch.empty((n + 15) // 16, 2, dtype=torch.float64, device=dev)  # (16-byte aligned)
    value = torch.empty((), dtype=torch.float32, device=dev)
    _launch_on(lib, "ddrr_recon_tv3d", dev, (
        volume.data_ptr(), *dims, *spacing, _TV_MODES[mode], float(eps), _ptr(grad), int(bool(accumulate)),
        float(weight), _ptr(scale), ws.data_ptr(), ws.numel() * 8, value.data_ptr()))
    return value


def volume_adam_step(param, grad, exp_avg, exp_avg_sq, step, *, lr, betas=(0.9, 0.999), eps=1e-8, lower=None,
                     upper=None, maximize=False):
    """One Adam step of `param` (any shape, fp32, contiguous, on the device) in place, then its projection
    onto [lower, upper] (None = no bound), in one pass (include/diffdrr_recon_hip.h ddrr_recon_adam_step:
    torch.optim.Adam's update; `step` is a 1-element float tensor on the device, incremented there)."""
    _check_volume_like("volume_adam_step: param", param)
    _require_gpu(param)
    for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _check_volume_like(f"volume_adam_step: {name}", t, param)
    if (not torch.is_tensor(step) or step.dtype != torch.float32 or step.numel() != 1
            or step.device != param.device):
        raise ValueError("volume_adam_step: a 1-element float32 step counter on the parameter's device")
    lo = float("-inf") if lower is None else float(lower)
    hi = float("inf") if upper is None else float(upper)
    if not lo <= hi:
        raise ValueError(f"volume_adam_step: lower {lower} must be <= upper {upper}")
    if not (float(lr) >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and float(eps) >= 0.0):
        raise ValueError("volume_adam_step: invalid lr / betas / eps")
    if param.numel():
        _launch_on(_lib.get_recon_lib(), "ddrr_recon_adam_step", param.device, (
            param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), step.data_ptr(),
            param.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), lo, hi, int(bool(maximize))))


# ------------------------------------------------------------------ FDK initialisation (libdiffdrr_fbp_hip.so)
def _check_projections(name, images):
    if not torch.is_tensor(images) or images.dim() != 3:
        raise ValueError(f"{name}: (B, H, W) images expected")
    _check_volume_like(f"{name}: images", images)
    _require_gpu(images)
    if max(images.shape[1:]) > _lib.FBP_MAX_IMAGE_DIM:
        raise ValueError(f"{name}: images of at most {_lib.FBP_MAX_IMAGE_DIM} pixels a side, got {tuple(images.shape)}")


def fbp_filter(images, axis, taps, scale=1.0, *, u0=0.0, du=1.0, v0=0.0, dv=1.0, sdd=1.0, cosine_weight=False,
               out=None):
    """Cosine weighting and 1-D convolution of `images` (B, H, W) fp32 on the device in one pass
    (include/diffdrr_fbp_hip.h ddrr_fbp_filter): along the columns within a row (`axis` 0) or along the
    rows within a column (`axis` 1), `taps` (2 L - 1,) with lag 0 at index L - 1, L the filtered axis'
    length.  -> `out` (a new tensor unless given; never `images` itself)."""
    _check_projections("fbp_filter", images)
    if axis not in (0, 1):
        raise ValueError(f"fbp_filter: axis must be 0 (along columns) or 1 (along rows), not {axis!r}")
    B, H, W = (int(d) for d in images.shape)
    if images.numel() > 2**31:
        raise ValueError(f"fbp_filter: at most 2^31 pixels, got {tuple(images.shape)}")
    L = W if axis == 0 else H
    _check_volume_like("fbp_filter: taps", taps)
    if taps.device != images.device or tuple(taps.shape) != (max(2 * L - 1, 0),):
        raise ValueError(f"fbp_filter: taps of shape ({2 * L - 1},) on {images.device} expected, got "
                         f"{tuple(taps.shape)} on {taps.device}")
    if cosine_weight and not float(sdd) > 0.0:
        raise ValueError(f"fbp_filter: sdd must be > 0, not {sdd}")
    if out is None:
        out = torch.empty_like(images)
    else:
        _check_volume_like("fbp_filter: out", out, images)
    if images.numel():
        _launch_on(_lib.get_fbp_lib(), "ddrr_fbp_filter", images.device, (
            images.data_ptr(), B, H, W, int(axis), taps.data_ptr(), float(scale), float(u0), float(du), float(v0),
            float(dv), float(sdd), int(bool(cosine_weight)), out.data_ptr()))
    return out


def fbp_backproject(images, views, volume_shape=None, *, distance_weight=False, out=None, accumulate=False):
    """Voxel-driven backprojection of `images` (B, H, W) fp32 on the device into a (Dx, Dy, Dz) volume
    (include/diffdrr_fbp_hip.h ddrr_fbp_backproject): `views` (B, 16) holds per view the row-major 3 x 4
    matrix voxel index -> (col U, row U, U) and a weight.  `out`: the volume to write (or, with
    `accumulate`, to add to); a new one of `volume_shape` otherwise.  -> the volume."""
    _check_projections("fbp_backproject", images)
    B, H, W = (int(d) for d in images.shape)
    _check_volume_like("fbp_backproject: views", views)
    if views.device != images.device or tuple(views.shape) != (B, _lib.FBP_VIEW_FLOATS):
        raise ValueError(f"fbp_backproject: views of shape ({B}, {_lib.FBP_VIEW_FLOATS}) on {images.device} expected, "
                         f"got {tuple(views.shape)} on {views.device}")
    if B > _lib.FBP_MAX_VIEWS:
        raise ValueError(f"fbp_backproject: at most {_lib.FBP_MAX_VIEWS} views, got {B}")
    if out is None:
        if accumulate:
            raise ValueError("fbp_backproject: accumulate needs an out tensor")
        if volume_shape is None or len(volume_shape) != 3:
            raise ValueError("fbp_backproject: a (Dx, Dy, Dz) volume_shape or an out tensor expected")
        out = torch.empty(tuple(int(d) for d in volume_shape), dtype=torch.float32, device=images.device)
    else:
        _check_volume_like("fbp_backproject: out", out)
        if out.dim() != 3 or out.device != images.device or (
                volume_shape is not None and tuple(out.shape) != tuple(volume_shape)):
            raise ValueError(f"fbp_backproject: out must be a (Dx, Dy, Dz) volume on {images.device}, got "
                             f"{tuple(out.shape)} on {out.device}")
    if max(out.shape) > _lib.FBP_MAX_DIM or out.numel() > 2**34:
        raise ValueError(f"fbp_backproject: at most {_lib.FBP_MAX_DIM} voxels per axis and 2^34 in all, got "
                         f"{tuple(out.shape)}")
    if out.numel():
        _launch_on(_lib.get_fbp_lib(), "ddrr_fbp_backproject", images.device, (
            images.data_ptr(), B, H, W, views.data_ptr(), int(bool(distance_weight)), out.data_ptr(),
            *(int(d) for d in out.shape), int(bool(accumulate))))
    return out


# ------------------------------------------------- Levenberg-Marquardt registration: what the four libraries share
def _lm_workspace(nbytes, poses, sums, device):
    """The (uninitialised) (poses, G, sums) float64 partial sums of ``nbytes`` bytes, as a library's query sized it."""
    n = int(nbytes) // 8
    return torch.empty(n, dtype=torch.float64, device=device).view(poses, -1, sums) if n else \
        torch.empty(poses, 0, sums, dtype=torch.float64, device=device)


def _check_lm_ws(name, ws, workspace, *shape, sums=None):
    """``ws`` is what ``workspace(*shape, device)`` (the family's ``<family>_workspace``, ``name`` being
    ``<family>_<entry>``) returns, as far as every family looks; with ``sums`` (wmvlm's own look) its three axes and
    the last of them too"""
    if ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() != workspace(*shape, "meta").numel() \
            or (sums is not None and (ws.dim() != 3 or ws.shape[-1] != sums)):
        raise ValueError(f"{name}: ws must be what {name.split('_')[0]}_workspace("
                         f"{'B, N' if len(shape) == 2 else 'S, V, N'}, device) returns")


def _check_lm_image(name, t, what, rows, N):
    """``t`` (the fixed image or the weight) is a float32 (r, N) tensor with r one of ``rows``: (1, B) for one row
    shared by the B poses or one each, (V,) for one per view"""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] not in rows or t.shape[1] != N or t.dtype != torch.float32:
        expected = f"of shape (1 | {rows[1]}, {N})" if len(rows) == 2 else f"per view, ({rows[0]}, {N}),"
        raise ValueError(f"{name}: a float32 {what} {expected} expected, got "
                         f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} {getattr(t, 'dtype', '')}")


def _check_lm_devices(name, dev, *named):
    for what, t in named:
        if t.device != dev:
            raise ValueError(f"{name}: {what} must live on the poses' device ({dev}), got {t.device}")


def _check_lm_state(name, rot, xyz, state, B="B"):
    """the step's own tensors: (B, 3) parameters, written in place, and the (B, 40) state"""
    n = rot.shape[0]
    for t in (rot, xyz):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != (n, 3):
            raise ValueError(f"{name}: contiguous float32 ({B}, 3) pose parameters")
    if state.dtype != torch.float64 or not state.is_contiguous() or state.shape != (n, _lib.LM_STATE_DOUBLES):
        raise ValueError(f"{name}: state must be a contiguous float64 ({B}, {_lib.LM_STATE_DOUBLES}) tensor")


def _check_lm_hyper(name, ncc_eps, up, down, damping_min, damping_max):
    if not (up > 1.0 and 0.0 < down < 1.0 and 0.0 < damping_min <= damping_max < float("inf") and ncc_eps >= 0.0):
        raise ValueError(f"{name}: up > 1, 0 < down < 1, 0 < damping_min <= damping_max < inf, ncc_eps >= 0 expected")


def _check_lm_views_out(name, S, V, dev, **outs):
    """the optional per-view outputs of a multi-view step: (tensor, dtype) by name"""
    for what, (t, dtype) in outs.items():
        if t is not None and (t.dtype != dtype or not t.is_contiguous() or t.shape != (S, V) or t.device != dev):
            raise ValueError(f"{name}: {what} must be a contiguous {str(dtype)[6:]} ({S}, {V}) tensor on the poses' "
                             "device")


def _lm_views(name, rot, xyz, reorient_v, *P, max_poses=_lib.MVLM_MAX_POSES):
    """(S, V) of (S, 3) parameters and (V, 3, 4) float32 reorients; given the detector points ``P`` -- (N, 3) shared
    by the views (stride 0) or (V, N, 3) (stride 3 N) -- (S, V, N, P_stride), everything on the poses' device;
    refuses what the entries would misread."""
    S = rot.shape[0]
    for t in (rot, xyz):
        if t.dtype != torch.float32 or t.shape != (S, 3):
            raise ValueError(f"{name}: float32 (S, 3) pose parameters expected, got {tuple(t.shape)} {t.dtype}")
    if reorient_v.dim() != 3 or reorient_v.shape[0] < 1 or tuple(reorient_v.shape[1:]) != (3, 4) \
            or reorient_v.dtype != torch.float32:
        raise ValueError(f"{name}: reorient_v must be a float32 (V, 3, 4) tensor with V >= 1, got "
                         f"{tuple(reorient_v.shape)} {reorient_v.dtype}")
    V = reorient_v.shape[0]
    if S * V > max_poses:
        raise ValueError(f"{name}: at most {max_poses} poses (S * V), got {S} * {V}")
    if not P:
        return S, V
    P, = P
    if not torch.is_tensor(P) or P.dtype != torch.float32 or P.dim() not in (2, 3) or P.shape[-1] != 3 \
            or (P.dim() == 3 and P.shape[0] != V):
        raise ValueError(f"{name}: the detector points must be float32 (N, 3), shared by the views, or ({V}, N, 3), "
                         f"got {tuple(P.shape) if torch.is_tensor(P) else type(P).__name__} {getattr(P, 'dtype', '')}")
    for what, t in (("xyz", xyz), ("reorient_v", reorient_v), ("detector points", P)):
        if t.device != rot.device:
            raise ValueError(f"{name}: {what} must live on the poses' device ({rot.device}), got {t.device}")
    N = P.shape[-2]
    return S, V, N, (3 * N if P.dim() == 3 else 0)


def _lm_raygen(name, launch, rot, xyz, axes, reorient_v, Ainv, P, P_stride, S, V, N, clear, clear_launch_ws):
    """The multi-view ray generation ``ddrr_<name>`` (``P_stride``: the run of arguments behind ``P``, () or (stride,))
    -> (Mw (S V, 3, 4), source_v (S V, 1, 3), target_v (S V, N, 3), img (S V, N))"""
    B = S * V
    rot, xyz, reorient_v, Ainv, P = (t.contiguous() for t in (rot, xyz, reorient_v, Ainv, P))
    dev = rot.device
    Mw = torch.empty(B, 3, 4, dtype=torch.float32, device=dev)
    source = torch.empty(B, 1, 3, dtype=torch.float32, device=dev)
    target = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    img = torch.empty(B, N, dtype=torch.float32, device=dev)
    if not _empty(B, N):
        launch("ddrr_" + name, dev, rot.data_ptr(), xyz.data_ptr(), *axes, reorient_v.data_ptr(), Ainv.data_ptr(),
               P.data_ptr(), *P_stride, S, V, N, Mw.data_ptr(), source.data_ptr(), target.data_ptr(), img.data_ptr(),
               _ptr(clear), 0 if clear is None else clear.numel(), _ptr(clear_launch_ws))
    elif clear is not None or clear_launch_ws is not None:
        raise ValueError(f"{name}: nothing is launched for an empty batch, nothing is cleared")
    return Mw, source, target, img


# ------------------------------------------------- Levenberg-Marquardt registration (libdiffdrr_lm_hip.so)
def _launch_lm(name, device, *args):
    """:func:`_launch` through the Levenberg-Marquardt library."""
    _launch_on(_lib.get_lm_lib(), name, device, args)


def _query_lm(name, *args):
    return _lib.get_lm_lib().query(name, *args)


def lm_workspace(B, N, device):
    """The (uninitialised) per-workgroup partial sums of :func:`lm_normal_sums` for B poses of N rays:
    (B, ceil(N / 1024), 44) float64."""
    return _lm_workspace(_query_lm("ddrr_lm_workspace_bytes", int(B), int(N)), B, _lib.LM_SUMS, device)


def lm_state(B, damping, device):
    """A fresh per-pose state of :func:`lm_step` (include/diffdrr_lm_hip.h): (B, 40) float64, zero but
    for the damping."""
    state = torch.zeros(B, _lib.LM_STATE_DOUBLES, dtype=torch.float64, device=device)
    state[:, 34] = float(damping)
    return state


def lm_normal_sums(aux, fixed, source, Mw, Ainv, P, rot, xyz, axes, reorient34, *, eps=1e-8, with_img_path=True,
                   ws=None, want_jacobian=False):
    """The 44 normal-equations sums of every rendered pose from the brick kernel's blocked record ``aux``
    (include/diffdrr_lm_hip.h ddrr_lm_normal_sums; ``fixed`` ((B | 1), N); the rest as
    :func:`pose_raygen_forward` made them) -> (ws (B, G, 44) float64 per-workgroup partials,
    jac (B, N, 6) float32 | None)."""
    _require_gpu(rot)
    B, N = rot.shape[0], P.shape[0]
    _check_lm_image("lm_normal_sums", fixed, "fixed image", (1, B), N)
    if B > _lib.LM_MAX_POSES:
        raise ValueError(f"lm_normal_sums: at most {_lib.LM_MAX_POSES} poses, got {B}")
    fixed, source = fixed.contiguous(), source.contiguous()
    held, chain = _pose_chain(Mw, Ainv, P, rot, xyz, axes, reorient34)
    dev = rot.device
    if ws is None:
        ws = lm_workspace(B, N, dev)
    else:
        _check_lm_ws("lm_normal_sums", ws, lm_workspace, B, N)
    jac = torch.empty(B, N, 6, dtype=torch.float32, device=dev) if want_jacobian else None
    if B and N:
        _launch_lm("ddrr_lm_normal_sums", dev, aux.data_ptr(), fixed.data_ptr(),
                   0 if (fixed.shape[0] == 1 and B != 1) else N, source.data_ptr(), *chain, B, N, float(eps),
                   int(bool(with_img_path)), ws.data_ptr(), _ptr(jac))
    return ws, jac


def lm_step(ws, state, rot, xyz, N, *, ncc_eps=1e-5, up=4.0, down=1.0 / 3.0, damping_min=1e-7, damping_max=1e6,
            out=None):
    """Accept or reject the rendered poses against ``state``, solve the damped normal equations of the best
    ones and write the next trial poses into ``rot``, ``xyz`` IN PLACE (include/diffdrr_lm_hip.h
    ddrr_lm_step) -> the best NCC per pose (B,) float32."""
    _require_gpu(rot)
    B = rot.shape[0]
    _check_lm_state("lm_step", rot, xyz, state)
    _check_lm_ws("lm_step", ws, lm_workspace, B, N)
    _check_lm_hyper("lm_step", ncc_eps, up, down, damping_min, damping_max)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=rot.device)
    if B:
        _launch_lm("ddrr_lm_step", rot.device, ws.data_ptr(), state.data_ptr(), rot.data_ptr(), xyz.data_ptr(), B,
                   int(N), float(ncc_eps), float(up), float(down), float(damping_min), float(damping_max),
                   out.data_ptr())
    return out


# ------------------------------------------------- weighted Levenberg-Marquardt (libdiffdrr_wlm_hip.so)
def _launch_wlm(name, device, *args):
    """:func:`_launch` through the weighted Levenberg-Marquardt library."""
    _launch_on(_lib.get_wlm_lib(), name, device, args)


def _query_wlm(name, *args):
    return _lib.get_wlm_lib().query(name, *args)


def wlm_workspace(B, N, device):
    """The (uninitialised) per-workgroup partial sums of :func:`wlm_normal_sums` for B poses of N rays:
    (B, ceil(N / 1024), 45) float64."""
    return _lm_workspace(_query_wlm("ddrr_wlm_workspace_bytes", int(B), int(N)), B, _lib.WLM_SUMS, device)


def wlm_normal_sums(aux, fixed, weight, *, source, Mw, Ainv, P, rot, xyz, axes, reorient34, eps=1e-8,
                    with_img_path=True, ws=None, want_jacobian=False):
    """The 45 weighted normal-equations sums of every rendered pose from the brick kernel's blocked record ``aux``
    (include/diffdrr_wlm_hip.h ddrr_wlm_normal_sums; ``fixed`` and ``weight`` ((B | 1), N) float32, weights >= 0
    and finite -- not looked for here; the rest as :func:`pose_raygen_forward` made them)
    -> (ws (B, G, 45) float64 per-workgroup partials, jac (B, N, 6) float32 | None)."""
    _require_gpu(rot)
    B, N = rot.shape[0], P.shape[0]
    dev = rot.device
    _check_lm_image("wlm_normal_sums", fixed, "fixed image", (1, B), N)
    _check_lm_image("wlm_normal_sums", weight, "weight", (1, B), N)
    _check_lm_devices("wlm_normal_sums", dev, ("the fixed image", fixed), ("the weight", weight))
    if B > _lib.WLM_MAX_POSES:
        raise ValueError(f"wlm_normal_sums: at most {_lib.WLM_MAX_POSES} poses, got {B}")
    fixed, weight, source = fixed.contiguous(), weight.contiguous(), source.contiguous()
    held, chain = _pose_chain(Mw, Ainv, P, rot, xyz, axes, reorient34)
    if ws is None:
        ws = wlm_workspace(B, N, dev)
    else:
        _check_lm_ws("wlm_normal_sums", ws, wlm_workspace, B, N)
    jac = torch.empty(B, N, 6, dtype=torch.float32, device=dev) if want_jacobian else None
    if B and N:
        _launch_wlm("ddrr_wlm_normal_sums", dev, aux.data_ptr(), fixed.data_ptr(),
                    0 if (fixed.shape[0] == 1 and B != 1) else N, weight.data_ptr(),
                    0 if (weight.shape[0] == 1 and B != 1) else N, source.data_ptr(), *chain, B, N, float(eps),
                    int(bool(with_img_path)), ws.data_ptr(), _ptr(jac))
    return ws, jac


def wlm_step(ws, state, rot, xyz, N, *, ncc_eps=1e-5, up=4.0, down=1.0 / 3.0, damping_min=1e-7, damping_max=1e6,
             out=None):
    """:func:`lm_step` on the weighted sums of :func:`wlm_normal_sums` (include/diffdrr_wlm_hip.h ddrr_wlm_step):
    the same state (:func:`lm_state`), whose column 37 takes the sum of the weights of the render just judged
    -> the best weighted NCC per pose (B,) float32."""
    _require_gpu(rot)
    B = rot.shape[0]
    _check_lm_state("wlm_step", rot, xyz, state)
    _check_lm_ws("wlm_step", ws, wlm_workspace, B, N)
    _check_lm_hyper("wlm_step", ncc_eps, up, down, damping_min, damping_max)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=rot.device)
    if B:
        _launch_wlm("ddrr_wlm_step", rot.device, ws.data_ptr(), state.data_ptr(), rot.data_ptr(), xyz.data_ptr(), B,
                    int(N), float(ncc_eps), float(up), float(down), float(damping_min), float(damping_max),
                    out.data_ptr())
    return out


# ------------------------------------------------- multi-view Levenberg-Marquardt (libdiffdrr_mvlm_hip.so)
def _launch_mvlm(name, device, *args):
    """:func:`_launch` through the multi-view Levenberg-Marquardt library."""
    _launch_on(_lib.get_mvlm_lib(), name, device, args)


def _query_mvlm(name, *args):
    return _lib.get_mvlm_lib().query(name, *args)


def mvlm_workspace(S, V, N, device):
    """The (uninitialised) per-workgroup partial sums of :func:`mvlm_normal_sums` for S starts seen from V views
    with N rays: (S * V, ceil(N / 1024), 44) float64."""
    return _lm_workspace(_query_mvlm("ddrr_mvlm_workspace_bytes", int(S), int(V), int(N)), S * V, _lib.MVLM_SUMS,
                         device)


def mvlm_raygen(rot, xyz, axes, reorient_v, Ainv, P, *, clear=None, clear_launch_ws=None):
    """:func:`pose_raygen_forward` for S starts seen from V views in one launch (include/diffdrr_mvlm_hip.h
    ddrr_mvlm_raygen): pose ``b = s * V + v`` is the Euler pose (rot[s], xyz[s]) with the reorient ``reorient_v[v]``
    -> (Mw (S V, 3, 4), source_v (S V, 1, 3), target_v (S V, N, 3), img (S V, N)).  ``clear`` and ``clear_launch_ws``
    as there."""
    _require_gpu(rot)
    S, V = _lm_views("mvlm_raygen", rot, xyz, reorient_v)
    return _lm_raygen("mvlm_raygen", _launch_mvlm, rot, xyz, axes, reorient_v, Ainv, P, (), S, V, P.shape[0], clear,
                      clear_launch_ws)


def mvlm_normal_sums(aux, fixed, source, Mw, Ainv, P, rot, xyz, axes, reorient_v, *, eps=1e-8, with_img_path=True,
                     ws=None, want_jacobian=False):
    """The 44 normal-equations sums of the S * V rendered poses from the brick kernel's blocked record ``aux``
    (include/diffdrr_mvlm_hip.h ddrr_mvlm_normal_sums; ``fixed`` (V, N) float32: one image per view; ``rot``,
    ``xyz`` (S, 3); ``reorient_v`` (V, 3, 4); the rest as :func:`mvlm_raygen` made them)
    -> (ws (S V, G, 44) float64 per-workgroup partials, jac (S V, N, 6) float32 | None)."""
    _require_gpu(rot)
    S, V = _lm_views("mvlm_normal_sums", rot, xyz, reorient_v)
    N, B = P.shape[0], S * V
    dev = rot.device
    _check_lm_image("mvlm_normal_sums", fixed, "fixed image", (V,), N)
    _check_lm_devices("mvlm_normal_sums", dev, ("the fixed images", fixed))
    if Mw.shape[0] != B or source.shape[0] != B:
        raise ValueError(f"mvlm_normal_sums: Mw and source of {B} poses (S * V) expected, got {Mw.shape[0]} and "
                         f"{source.shape[0]}")
    fixed, source = fixed.contiguous(), source.contiguous()
    held, chain = _pose_chain(Mw, Ainv, P, rot, xyz, axes, reorient_v)
    if ws is None:
        ws = mvlm_workspace(S, V, N, dev)
    else:
        _check_lm_ws("mvlm_normal_sums", ws, mvlm_workspace, S, V, N)
    jac = torch.empty(B, N, 6, dtype=torch.float32, device=dev) if want_jacobian else None
    if B and N:
        _launch_mvlm("ddrr_mvlm_normal_sums", dev, aux.data_ptr(), fixed.data_ptr(), source.data_ptr(), *chain, S, V,
                     N, float(eps), int(bool(with_img_path)), ws.data_ptr(), _ptr(jac))
    return ws, jac


def mvlm_step(ws, state, rot, xyz, V, N, *, ncc_eps=1e-5, up=4.0, down=1.0 / 3.0, damping_min=1e-7, damping_max=1e6,
              out=None, ncc_views=None):
    """:func:`lm_step` for S starts on the sums of their V views (include/diffdrr_mvlm_hip.h ddrr_mvlm_step): the
    views' normal equations are added, the mean NCC is judged against ``state`` ((S, 40), :func:`lm_state`), the
    next trial is written into ``rot``, ``xyz`` (S, 3) IN PLACE -> the best mean NCC per start (S,) float32.
    ``ncc_views`` ((S, V) float32, optional) receives the NCC of every view of the render just judged."""
    _require_gpu(rot)
    S, V = rot.shape[0], int(V)
    if V < 1 or S * V > _lib.MVLM_MAX_POSES:
        raise ValueError(f"mvlm_step: V >= 1 and at most {_lib.MVLM_MAX_POSES} poses (S * V) expected, got {S} * {V}")
    _check_lm_state("mvlm_step", rot, xyz, state, "S")
    _check_lm_ws("mvlm_step", ws, mvlm_workspace, S, V, N)
    _check_lm_hyper("mvlm_step", ncc_eps, up, down, damping_min, damping_max)
    _check_lm_views_out("mvlm_step", S, V, rot.device, ncc_views=(ncc_views, torch.float32))
    if out is None:
        out = torch.empty(S, dtype=torch.float32, device=rot.device)
    if S:
        _launch_mvlm("ddrr_mvlm_step", rot.device, ws.data_ptr(), state.data_ptr(), rot.data_ptr(), xyz.data_ptr(), S,
                     V, int(N), float(ncc_eps), float(up), float(down), float(damping_min), float(damping_max),
                     out.data_ptr(), _ptr(ncc_views))
    return out


# ------------------------------- weighted multi-view Levenberg-Marquardt (libdiffdrr_wmvlm_hip.so)
def _launch_wmvlm(name, device, *args):
    """:func:`_launch` through the weighted multi-view Levenberg-Marquardt library."""
    _launch_on(_lib.get_wmvlm_lib(), name, device, args)


def _query_wmvlm(name, *args):
    return _lib.get_wmvlm_lib().query(name, *args)


def wmvlm_workspace(S, V, N, device):
    """The (uninitialised) per-workgroup partial sums of :func:`wmvlm_normal_sums` for S starts seen from V views
    with N rays: (S * V, ceil(N / 1024), 45) float64."""
    return _lm_workspace(_query_wmvlm("ddrr_wmvlm_workspace_bytes", int(S), int(V), int(N)), S * V, _lib.WMVLM_SUMS,
                         device)


def wmvlm_raygen(rot, xyz, axes, reorient_v, Ainv, P, *, clear=None, clear_launch_ws=None):
    """:func:`mvlm_raygen` with a detector per view (include/diffdrr_wmvlm_hip.h ddrr_wmvlm_raygen): pose
    ``b = s * V + v`` is the Euler pose (rot[s], xyz[s]) with the reorient ``reorient_v[v]`` on the detector points
    ``P[v]`` (``P`` (V, N, 3)) or ``P`` ((N, 3), shared by the views)
    -> (Mw (S V, 3, 4), source_v (S V, 1, 3), target_v (S V, N, 3), img (S V, N)).  ``clear`` and ``clear_launch_ws``
    as there."""
    _require_gpu(rot)
    S, V, N, P_stride = _lm_views("wmvlm_raygen", rot, xyz, reorient_v, P, max_poses=_lib.WMVLM_MAX_POSES)
    return _lm_raygen("wmvlm_raygen", _launch_wmvlm, rot, xyz, axes, reorient_v, Ainv, P, (P_stride,), S, V, N, clear,
                      clear_launch_ws)


def wmvlm_normal_sums(aux, fixed, weight, source, Mw, Ainv, P, rot, xyz, axes, reorient_v, *, eps=1e-8,
                      with_img_path=True, ws=None, want_jacobian=False):
    """The 45 weighted normal-equations sums of the S * V rendered poses from the brick kernel's blocked record
    ``aux`` (include/diffdrr_wmvlm_hip.h ddrr_wmvlm_normal_sums; ``fixed`` (V, N) float32: one image per view;
    ``weight`` ((1 | V), N) float32, >= 0 and finite -- not looked for here: one row shared by the views, or a row
    per view; ``P`` (N, 3) or (V, N, 3); ``rot``, ``xyz`` (S, 3); ``reorient_v`` (V, 3, 4); the rest as
    :func:`wmvlm_raygen` made them)
    -> (ws (S V, G, 45) float64 per-workgroup partials, jac (S V, N, 6) float32 | None)."""
    _require_gpu(rot)
    S, V, N, P_stride = _lm_views("wmvlm_normal_sums", rot, xyz, reorient_v, P,
                                      max_poses=_lib.WMVLM_MAX_POSES)
    B = S * V
    dev = rot.device
    _check_lm_image("wmvlm_normal_sums", fixed, "fixed image", (V,), N)
    _check_lm_image("wmvlm_normal_sums", weight, "weight", (1, V), N)
    _check_lm_devices("wmvlm_normal_sums", dev, ("the fixed images", fixed), ("the weight", weight))
    if Mw.shape[0] != B or source.shape[0] != B:
        raise ValueError(f"wmvlm_normal_sums: Mw and source of {B} poses (S * V) expected, got {Mw.shape[0]} and "
                         f"{source.shape[0]}")
    fixed, weight, source = fixed.contiguous(), weight.contiguous(), source.contiguous()
    Mw, Ainv, P, rot, xyz, reorient_v = (t.contiguous() for t in (Mw, Ainv, P, rot, xyz, reorient_v))
    if ws is None:
        ws = wmvlm_workspace(S, V, N, dev)
    else:
        _check_lm_ws("wmvlm_normal_sums", ws, wmvlm_workspace, S, V, N, sums=_lib.WMVLM_SUMS)
    jac = torch.empty(B, N, 6, dtype=torch.float32, device=dev) if want_jacobian else None
    if B and N:
        _launch_wmvlm("ddrr_wmvlm_normal_sums", dev, aux.data_ptr(), fixed.data_ptr(), weight.data_ptr(),
                      0 if weight.shape[0] == 1 else N, source.data_ptr(), Mw.data_ptr(), Ainv.data_ptr(),
                      P.data_ptr(), P_stride, rot.data_ptr(), xyz.data_ptr(), *axes, reorient_v.data_ptr(), S, V, N,
                      float(eps), int(bool(with_img_path)), ws.data_ptr(), _ptr(jac))
    return ws, jac


def wmvlm_step(ws, state, rot, xyz, V, N, *, ncc_eps=1e-5, up=4.0, down=1.0 / 3.0, damping_min=1e-7, damping_max=1e6,
               out=None, ncc_views=None, sw_views=None):
    """:func:`wlm_step` for S starts on the weighted sums of their V views (include/diffdrr_wmvlm_hip.h
    ddrr_wmvlm_step): the non-empty views' normal equations are added, the mean of their NCC weighted by their sums
    of weights is judged against ``state`` ((S, 40), :func:`lm_state`; column 37 takes the start's sum of weights),
    the next trial is written into ``rot``, ``xyz`` (S, 3) IN PLACE -> the best such NCC per start (S,) float32.
    ``ncc_views`` ((S, V) float32) and ``sw_views`` ((S, V) float64), both optional, receive the NCC and the sum of
    weights of every view of the render just judged."""
    _require_gpu(rot)
    S, V = rot.shape[0], int(V)
    if V < 1 or S * V > _lib.WMVLM_MAX_POSES:
        raise ValueError(f"wmvlm_step: V >= 1 and at most {_lib.WMVLM_MAX_POSES} poses (S * V) expected, got "
                         f"{S} * {V}")
    _check_lm_state("wmvlm_step", rot, xyz, state, "S")
    _check_lm_ws("wmvlm_step", ws, wmvlm_workspace, S, V, N, sums=_lib.WMVLM_SUMS)
    # (the other three steps do not look at the devices)
    _check_lm_devices("wmvlm_step", rot.device, ("xyz", xyz), ("state", state), ("ws", ws))
    _check_lm_hyper("wmvlm_step", ncc_eps, up, down, damping_min, damping_max)
    _check_lm_views_out("wmvlm_step", S, V, rot.device, ncc_views=(ncc_views, torch.float32),
                        sw_views=(sw_views, torch.float64))
    if out is None:
        out = torch.empty(S, dtype=torch.float32, device=rot.device)
    if S:
        _launch_wmvlm("ddrr_wmvlm_step", rot.device, ws.data_ptr(), state.data_ptr(), rot.data_ptr(), xyz.data_ptr(),
                      S, V, int(N), float(ncc_eps), float(up), float(down), float(damping_min), float(damping_max),
                      out.data_ptr(), _ptr(ncc_views), _ptr(sw_views))
    return out


# ------------------------------------------------- weighted (masked) NCC (libdiffdrr_wncc_hip.so)
def _launch_wncc(name, device, *args):
    """:func:`_launch` through the weighted NCC library."""
    _launch_on(_lib.get_wncc_lib(), name, device, args)


def _query_wncc(name, *args):
    return _lib.get_wncc_lib().query(name, *args)


_wncc_ws = {}  # (device, stream, B, N) -> workspace of ddrr_wncc_* (uninitialised: per-workgroup partials)


def wncc_workspace(B, N, device):
    """The per-workgroup partials of the weighted NCC entries for B pairs of N pixels (include/diffdrr_wncc_hip.h):
    uninitialised, every call writes what it reads, so one buffer per (device, stream, B, N) serves every call on
    that stream.  ``GraphedIteration`` creates it for its capture stream before it captures."""
    dev = torch.device(device)
    sid = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    key = (dev, sid, int(B), int(N))
    ws = _wncc_ws.get(key)
    if ws is None:
        n = int(_query_wncc("ddrr_wncc_workspace_bytes", int(B), int(N)))
        ws = _wncc_ws[key] = torch.empty(n // 8, dtype=torch.float64, device=dev)
    return ws


def _weight_rows(name, w, B, N):
    if w.dim() != 2 or w.shape[1] != N or w.shape[0] not in (1, B) or w.dtype != torch.float32:
        raise ValueError(f"{name}: the weight has shape {tuple(w.shape)} {w.dtype}: float32 ({B}, {N}), or (1, {N}) "
                         f"for one weight shared by the batch, expected")


def _wncc_pair(name, x1, w, B, N):
    """The checks and strides the four entries share -> (x1, x1_stride, w, w_stride)."""
    _fixed_rows(name, x1, B, N)
    _weight_rows(name, w, B, N)
    if B > _lib.WNCC_MAX_POSES:
        raise ValueError(f"{name}: at most {_lib.WNCC_MAX_POSES} pairs, got {B}")
    return (x1.contiguous(), 0 if (x1.shape[0] == 1 and B != 1) else N,
            w.contiguous(), 0 if (w.shape[0] == 1 and B != 1) else N)


def wncc_forward(x1, x2, w, eps):
    """Weighted NCC (include/diffdrr_wncc_hip.h) of x2 (B, N) with x1 ((B | 1), N) under the weights w ((B | 1), N),
    >= 0 and finite; pixels with w == 0 are not read into any sum.  -> (ncc (B), stats (B, 6))"""
    B, N = x2.shape
    x1, s1, w, sw = _wncc_pair("wncc_forward", x1, w, B, N)
    _require_gpu(x2)
    x2 = x2.contiguous()
    ncc = torch.empty(B, dtype=torch.float32, device=x2.device)
    stats = torch.empty(B, _lib.WNCC_STATS, dtype=torch.float32, device=x2.device)
    if B and N:
        _launch_wncc("ddrr_wncc_forward", x2.device, x1.data_ptr(), s1, x2.data_ptr(), w.data_ptr(), sw, B, N,
                     float(eps), wncc_workspace(B, N, x2.device).data_ptr(), ncc.data_ptr(), stats.data_ptr())
    return ncc, stats


def wncc_backward(x1, x2, w, stats, g_out, want_x1, want_x2):
    """(g_x1 | None, g_x2 | None), each (B, N), of sum_b g_out[b] ncc_b; a shared x1 gets no gradient here."""
    B, N = x2.shape
    x1, s1, w, sw = _wncc_pair("wncc_backward", x1, w, B, N)
    x2 = x2.contiguous()
    g_out, g_stride = _batch_grad(g_out, B)
    g_x2 = torch.empty_like(x2) if want_x2 else None
    g_x1 = torch.empty_like(x2) if (want_x1 and s1 == N) else None
    if B and N:
        _launch_wncc("ddrr_wncc_backward", x2.device, x1.data_ptr(), s1, x2.data_ptr(), w.data_ptr(), sw,
                     stats.data_ptr(), g_out.data_ptr(), g_stride, B, N, _ptr(g_x1), _ptr(g_x2))
    return g_x1, g_x2


def siddon_wncc_forward(aux, img, x1, w, eps, *, want_image=False, want_sum=False):
    """:func:`siddon_ncc_forward` under per-pixel weights w ((B | 1), N): the image is formed from the blocked
    record on the fly.  -> (ncc (B), stats (B, 6), image (B, N) | None[, sum of the B values (0-dim), with
    ``want_sum``: added in pose order by the fold's own launch])"""
    B, N = img.shape
    _blocked_record_only("siddon_wncc_forward", aux, B, N)
    x1, s1, w, sw = _wncc_pair("siddon_wncc_forward", x1, w, B, N)
    img = img.contiguous()
    dev = img.device
    ncc = torch.empty(B, dtype=torch.float32, device=dev)
    stats = torch.empty(B, _lib.WNCC_STATS, dtype=torch.float32, device=dev)
    out = torch.empty(B, N, dtype=torch.float32, device=dev) if want_image else None
    total = (torch.empty((), dtype=torch.float32, device=dev) if B else
             torch.zeros((), dtype=torch.float32, device=dev)) if want_sum else None
    if B:
        _launch_wncc("ddrr_wncc_siddon_forward", dev, aux.data_ptr(), img.data_ptr(), x1.data_ptr(), s1,
                     w.data_ptr(), sw, B, N, float(eps), wncc_workspace(B, N, dev).data_ptr(), ncc.data_ptr(),
                     stats.data_ptr(), _ptr(out), _ptr(total))
    return (ncc, stats, out, total) if want_sum else (ncc, stats, out)


def siddon_wncc_backward_pose(aux, x1, w, stats, g_out, source, Mw, Ainv, P, rot, xyz, axes, reorient34, *,
                              eps=1e-8, with_img_path=True):
    """(g_rot (B,3), g_xyz (B,3)) of sum_b g_out[b] ncc_b of :func:`siddon_wncc_forward`: the weighted NCC
    backward, the record's ray gradients, the ray generation's adjoint and pose_euler_backward in two launches."""
    B, N = rot.shape[0], P.shape[0]
    _blocked_record_only("siddon_wncc_backward_pose", aux, B, N)
    x1, s1, w, sw = _wncc_pair("siddon_wncc_backward_pose", x1, w, B, N)
    g_out, g_stride = _batch_grad(g_out, B)
    source = source.contiguous()
    held, chain = _pose_chain(Mw, Ainv, P, rot, xyz, axes, reorient34)
    dev = rot.device
    g_rot, g_xyz = _pose_grads(B, dev)
    if B:
        _launch_wncc("ddrr_wncc_siddon_backward_pose", dev, aux.data_ptr(), x1.data_ptr(), s1, w.data_ptr(), sw,
                     stats.data_ptr(), g_out.data_ptr(), g_stride, source.data_ptr(), *chain, B, N, float(eps),
                     int(bool(with_img_path)), wncc_workspace(B, N, dev).data_ptr(), g_rot.data_ptr(),
                     g_xyz.data_ptr())
    return g_rot, g_xyz


# ------------------------------------------------- free-form deformation (libdiffdrr_warp_hip.so)
_WARP_PADDING = {"zeros": _lib.WARP_PADDING_ZEROS, "border": _lib.WARP_PADDING_BORDER}


def _launch_warp(name, device, *args):
    """:func:`_launch` through the free-form deformation library."""
    _launch_on(_lib.get_warp_lib(), name, device, args)


def _query_warp(name, *args):
    return _lib.get_warp_lib().query(name, *args)


def _check_warp(name, shape, displacement, padding, **volumes):
    """The domain of include/diffdrr_warp_hip.h, each condition by name -> (dims, grid, padding code)."""
    if padding not in _WARP_PADDING:
        raise ValueError(f"{name}: padding must be 'zeros' or 'border', not {padding!r}")
    for what, t in (("displacement", displacement), *volumes.items()):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{name}: {what}: a float32 tensor expected, got "
                             f"{t.dtype if torch.is_tensor(t) else type(t).__name__}")
        if not on_device(t):
            raise ValueError(f"{name}: {what} is on {t.device}: the warp kernels run on the GPU only (the package "
                             "has no CPU fallback)")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous")
        if t.device != displacement.device:
            raise ValueError(f"{name}: {what} is on {t.device}, the displacement on {displacement.device}")
    dims = tuple(int(d) for d in shape)
    if len(dims) != 3:
        raise ValueError(f"{name}: a (Dx, Dy, Dz) volume expected, got shape {dims}")
    for what, t in volumes.items():
        if tuple(t.shape) != dims:
            raise ValueError(f"{name}: {what} has shape {tuple(t.shape)}, expected {dims}")
    if displacement.dim() != 4 or displacement.shape[0] != 3:
        raise ValueError(f"{name}: a (3, Gx, Gy, Gz) displacement lattice expected, got shape "
                         f"{tuple(displacement.shape)}")
    grid = tuple(int(g) for g in displacement.shape[1:])
    if max(dims) > _lib.WARP_MAX_DIM:
        raise ValueError(f"{name}: at most {_lib.WARP_MAX_DIM} voxels per axis, got {dims}")
    if dims[0] * dims[1] * dims[2] > 2**31:
        raise ValueError(f"{name}: at most 2^31 voxels, got {dims} (larger volumes are out of scope)")
    if any(g < 2 or g > d for g, d in zip(grid, dims)):
        raise ValueError(f"{name}: the lattice needs 2 <= G_a <= D_a nodes per axis, got {grid} for a volume of {dims}")
    return dims, grid, _WARP_PADDING[padding]


def warp_forward(volume, displacement, padding="zeros"):
    """W = V o (id + u), u the trilinear interpolation of the lattice ``displacement`` (3, Gx, Gy, Gz) in
    voxels (include/diffdrr_warp_hip.h ddrr_warp_forward) -> W, a new tensor of the volume's shape."""
    dims, grid, pad = _check_warp("warp_forward", getattr(volume, "shape", ()), displacement, padding, volume=volume)
    out = torch.empty_like(volume)
    _launch_warp("ddrr_warp_forward", volume.device, volume.data_ptr(), *dims, displacement.data_ptr(), *grid, pad,
                 out.data_ptr())
    return out


def warp_backward_displacement(volume, displacement, grad_out, padding="zeros"):
    """The lattice gradient of :func:`warp_forward` for the upstream ``grad_out`` (the volume's shape)
    (ddrr_warp_backward_displacement: no atomics, bitwise reproducible) -> (3, Gx, Gy, Gz)."""
    dims, grid, pad = _check_warp("warp_backward_displacement", getattr(volume, "shape", ()), displacement, padding,
                                  volume=volume, grad_out=grad_out)
    n = int(_query_warp("ddrr_warp_workspace_bytes", *dims, *grid))
    if n < 0:
        raise ValueError(f"warp_backward_displacement: a lattice of {grid} on a volume of {dims} needs more than "
                         "2^31 - 1 (cell, piece) workgroups")
    ws = torch.empty(n // 4, dtype=torch.float32, device=volume.device)
    out = torch.empty_like(displacement)
    _launch_warp("ddrr_warp_backward_displacement", volume.device, volume.data_ptr(), *dims, displacement.data_ptr(),
                 *grid, pad, grad_out.data_ptr(), ws.data_ptr(), n, out.data_ptr())
    return out


def warp_backward_volume(displacement, grad_out, padding="zeros"):
    """The volume gradient of :func:`warp_forward`: the trilinear scatter of ``grad_out`` (float atomics: not
    bitwise reproducible on the device; ddrr_warp_backward_volume) -> the volume's shape."""
    dims, grid, pad = _check_warp("warp_backward_volume", getattr(grad_out, "shape", ()), displacement, padding,
                                  grad_out=grad_out)
    out = torch.empty_like(grad_out)
    _launch_warp("ddrr_warp_backward_volume", grad_out.device, displacement.data_ptr(), *grid, *dims, pad,
                 grad_out.data_ptr(), out.data_ptr())
    return out


# ------------------------------------------------- cubic B-spline deformation (libdiffdrr_bspline_hip.so)
_BSPLINE_PADDING = {"zeros": _lib.BSPLINE_PADDING_ZEROS, "border": _lib.BSPLINE_PADDING_BORDER}


def _launch_bspline(name, device, *args):
    """:func:`_launch` through the cubic B-spline deformation library."""
    _launch_on(_lib.get_bspline_lib(), name, device, args)


def _query_bspline(name, *args):
    return _lib.get_bspline_lib().query(name, *args)


def _check_bspline(name, shape, displacement, padding, **volumes):
    """The domain of include/diffdrr_bspline_hip.h -- that of :func:`_check_warp`, each condition by name
    -> (dims, grid, padding code)."""
    dims, grid, _ = _check_warp(name, shape, displacement, padding, **volumes)
    return dims, grid, _BSPLINE_PADDING[padding]


def bspline_forward(volume, displacement, padding="zeros"):
    """W = V o (id + u), u the cubic B-spline with the coefficients ``displacement`` (3, Gx, Gy, Gz) in voxels
    (include/diffdrr_bspline_hip.h ddrr_bspline_forward; an approximating spline: u at a node is not the
    node's coefficient) -> W, a new tensor of the volume's shape."""
    dims, grid, pad = _check_bspline("bspline_forward", getattr(volume, "shape", ()), displacement, padding,
                                     volume=volume)
    out = torch.empty_like(volume)
    _launch_bspline("ddrr_bspline_forward", volume.device, volume.data_ptr(), *dims, displacement.data_ptr(), *grid,
                    pad, out.data_ptr())
    return out


def bspline_backward_displacement(volume, displacement, grad_out, padding="zeros"):
    """The coefficient gradient of :func:`bspline_forward` for the upstream ``grad_out`` (the volume's shape)
    (ddrr_bspline_backward_displacement: three gathers of fixed order, no atomics, bitwise reproducible)
    -> (3, Gx, Gy, Gz)."""
    dims, grid, pad = _check_bspline("bspline_backward_displacement", getattr(volume, "shape", ()), displacement,
                                     padding, volume=volume, grad_out=grad_out)
    n = int(_query_bspline("ddrr_bspline_workspace_bytes", *dims, *grid))
    ws = torch.empty(n // 4, dtype=torch.float32, device=volume.device)
    out = torch.empty_like(displacement)
    _launch_bspline("ddrr_bspline_backward_displacement", volume.device, volume.data_ptr(), *dims,
                    displacement.data_ptr(), *grid, pad, grad_out.data_ptr(), ws.data_ptr(), n, out.data_ptr())
    return out


def bspline_backward_volume(displacement, grad_out, padding="zeros"):
    """The volume gradient of :func:`bspline_forward`: the trilinear scatter of ``grad_out`` (float atomics: not
    bitwise reproducible on the device; ddrr_bspline_backward_volume) -> the volume's shape."""
    dims, grid, pad = _check_bspline("bspline_backward_volume", getattr(grad_out, "shape", ()), displacement,
                                     padding, grad_out=grad_out)
    out = torch.empty_like(grad_out)
    _launch_bspline("ddrr_bspline_backward_volume", grad_out.device, displacement.data_ptr(), *grid, *dims, pad,
                    grad_out.data_ptr(), out.data_ptr())
    return out


# ------------------------------------------------- Jacobian determinant (libdiffdrr_jacobian_hip.so)
_JACOBIAN_BASIS = {"linear": _lib.JACOBIAN_BASIS_LINEAR, "bspline": _lib.JACOBIAN_BASIS_BSPLINE}


def _launch_jacobian(name, device, *args):
    """:func:`_launch` through the Jacobian determinant library."""
    _launch_on(_lib.get_jacobian_lib(), name, device, args)


def _query_jacobian(name, *args):
    return _lib.get_jacobian_lib().query(name, *args)


def _check_jacobian(name, shape, displacement, basis, eps=None, **volumes):
    """The domain of include/diffdrr_jacobian_hip.h -- that of :func:`_check_warp`, the basis and ``eps`` in
    (0, 1], each condition by name -> (dims, grid, basis code)."""
    if basis not in _JACOBIAN_BASIS:
        raise ValueError(f"{name}: basis must be 'linear' or 'bspline', not {basis!r}")
    if eps is not None and not 0.0 < float(eps) <= 1.0:
        raise ValueError(f"{name}: eps must be in (0, 1], got {eps!r}")
    dims, grid, _ = _check_warp(name, shape, displacement, "zeros", **volumes)
    return dims, grid, _JACOBIAN_BASIS[basis]


def _jacobian_workspace(name, dims, grid, code, device):
    n = int(_query_jacobian("ddrr_jacobian_workspace_bytes", *dims, *grid, code))
    if n < 0:
        raise ValueError(f"{name}: a lattice of {grid} on a volume of {dims} needs more than 2^31 - 1 (cell, piece) "
                         "workgroups")
    return torch.empty((n + 7) // 8, dtype=torch.float64, device=device), n


def jacobian_determinant(displacement, shape, basis="linear"):
    """det(I + du/dx) at every voxel of a volume of ``shape`` for the lattice ``displacement`` (3, Gx, Gy, Gz) in
    voxels, and its statistics (ddrr_jacobian_determinant) -> (map of ``shape``, folded: one int64 on the device,
    range: (min, max) float32 on the device).  No host synchronisation."""
    dims, grid, code = _check_jacobian("jacobian_determinant", shape, displacement, basis)
    dev = displacement.device
    ws, n = _jacobian_workspace("jacobian_determinant", dims, grid, code, dev)
    out = torch.empty(dims, dtype=torch.float32, device=dev)
    folded = torch.empty(1, dtype=torch.int64, device=dev)
    rng = torch.empty(2, dtype=torch.float32, device=dev)
    _launch_jacobian("ddrr_jacobian_determinant", dev, displacement.data_ptr(), *grid, *dims, code, out.data_ptr(),
                     ws.data_ptr(), n, folded.data_ptr(), rng.data_ptr())
    return out, folded, rng


def jacobian_penalty(displacement, shape, basis="linear", eps=0.1):
    """The mean of psi(det) over the voxels and the statistics, with no map in memory (ddrr_jacobian_penalty)
    -> (penalty: one float64 on the device, folded, range) as :func:`jacobian_determinant`."""
    dims, grid, code = _check_jacobian("jacobian_penalty", shape, displacement, basis, eps)
    dev = displacement.device
    ws, n = _jacobian_workspace("jacobian_penalty", dims, grid, code, dev)
    penalty = torch.empty(1, dtype=torch.float64, device=dev)
    folded = torch.empty(1, dtype=torch.int64, device=dev)
    rng = torch.empty(2, dtype=torch.float32, device=dev)
    _launch_jacobian("ddrr_jacobian_penalty", dev, displacement.data_ptr(), *grid, *dims, code, float(eps),
                     ws.data_ptr(), n, penalty.data_ptr(), folded.data_ptr(), rng.data_ptr())
    return penalty, folded, rng


def jacobian_backward(displacement, shape, grad_out=None, basis="linear", eps=0.1):
    """The lattice gradient of the determinant map for the upstream ``grad_out`` (``shape``), or of the penalty
    (psi'(det) / N formed in the kernel) when ``grad_out`` is None (ddrr_jacobian_backward: no atomics, bitwise
    reproducible) -> (3, Gx, Gy, Gz)."""
    volumes = {} if grad_out is None else {"grad_out": grad_out}
    dims, grid, code = _check_jacobian("jacobian_backward", shape, displacement, basis, eps, **volumes)
    dev = displacement.device
    ws, n = _jacobian_workspace("jacobian_backward", dims, grid, code, dev)
    out = torch.empty_like(displacement)
    _launch_jacobian("ddrr_jacobian_backward", dev, displacement.data_ptr(), *grid, *dims, code, _ptr(grad_out),
                     float(eps), ws.data_ptr(), n, out.data_ptr())
    return out


# ------------------------------------------------- polyrigid deformation (libdiffdrr_polyrigid_hip.so)
_POLYRIGID_PADDING = {"zeros": _lib.POLYRIGID_PADDING_ZEROS, "border": _lib.POLYRIGID_PADDING_BORDER}


def _launch_polyrigid(name, device, *args):
    """:func:`_launch` through the polyrigid deformation library."""
    _launch_on(_lib.get_polyrigid_lib(), name, device, args)


def _query_polyrigid(name, *args):
    return _lib.get_polyrigid_lib().query(name, *args)


def _check_polyrigid(name, shape, twists, pitch, padding, **volumes):
    """The domain of include/diffdrr_polyrigid_hip.h, each condition by name
    -> (dims, grid, pitch as three floats, padding code)."""
    if padding not in _POLYRIGID_PADDING:
        raise ValueError(f"{name}: padding must be 'zeros' or 'border', not {padding!r}")
    for what, t in (("twists", twists), *volumes.items()):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{name}: {what}: a float32 tensor expected, got "
                             f"{t.dtype if torch.is_tensor(t) else type(t).__name__}")
        if not on_device(t):
            raise ValueError(f"{name}: {what} is on {t.device}: the polyrigid kernels run on the GPU only (the "
                             "package has no CPU fallback)")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous")
        if t.device != twists.device:
            raise ValueError(f"{name}: {what} is on {t.device}, the twists on {twists.device}")
    dims = tuple(int(d) for d in shape)
    if len(dims) != 3:
        raise ValueError(f"{name}: a (Dx, Dy, Dz) volume expected, got shape {dims}")
    for what, t in volumes.items():
        if tuple(t.shape) != dims:
            raise ValueError(f"{name}: {what} has shape {tuple(t.shape)}, expected {dims}")
    if twists.dim() != 4 or twists.shape[0] != 6:
        raise ValueError(f"{name}: a (6, Gx, Gy, Gz) twist lattice expected, got shape {tuple(twists.shape)}")
    grid = tuple(int(g) for g in twists.shape[1:])
    if max(dims) > _lib.POLYRIGID_MAX_DIM:
        raise ValueError(f"{name}: at most {_lib.POLYRIGID_MAX_DIM} voxels per axis, got {dims}")
    if dims[0] * dims[1] * dims[2] > 2**31:
        raise ValueError(f"{name}: at most 2^31 voxels, got {dims} (larger volumes are out of scope)")
    if any(g < 2 or g > d for g, d in zip(grid, dims)):
        raise ValueError(f"{name}: the lattice needs 2 <= G_a <= D_a nodes per axis, got {grid} for a volume of {dims}")
    pitch = tuple(float(h) for h in pitch)
    if len(pitch) != 3 or not all(0.0 < h < float("inf") for h in pitch):
        raise ValueError(f"{name}: the voxel pitch must be three positive finite numbers (mm), got {pitch}")
    return dims, grid, pitch, _POLYRIGID_PADDING[padding]


def polyrigid_forward(volume, twists, pitch=(1.0, 1.0, 1.0), padding="zeros"):
    """W = V o (id + u), u(x) = (exp(xi(x)) y - y) / pitch with xi the trilinear interpolation of the twist lattice
    ``twists`` (6, Gx, Gy, Gz) = (omega in radians, v in mm) and y the voxel's position in mm from the volume's
    centre (include/diffdrr_polyrigid_hip.h ddrr_polyrigid_forward) -> W, a new tensor of the volume's shape."""
    dims, grid, h, pad = _check_polyrigid("polyrigid_forward", getattr(volume, "shape", ()), twists, pitch, padding,
                                          volume=volume)
    out = torch.empty_like(volume)
    _launch_polyrigid("ddrr_polyrigid_forward", volume.device, volume.data_ptr(), *dims, twists.data_ptr(), *grid, *h,
                      pad, out.data_ptr())
    return out


def polyrigid_backward_twists(volume, twists, grad_out, pitch=(1.0, 1.0, 1.0), padding="zeros"):
    """The twist-lattice gradient of :func:`polyrigid_forward` for the upstream ``grad_out`` (the volume's shape)
    (ddrr_polyrigid_backward_twists: no atomics, bitwise reproducible) -> (6, Gx, Gy, Gz)."""
    dims, grid, h, pad = _check_polyrigid("polyrigid_backward_twists", getattr(volume, "shape", ()), twists, pitch,
                                          padding, volume=volume, grad_out=grad_out)
    n = int(_query_polyrigid("ddrr_polyrigid_workspace_bytes", *dims, *grid))
    if n < 0:
        raise ValueError(f"polyrigid_backward_twists: a lattice of {grid} on a volume of {dims} needs more than "
                         "2^31 - 1 (cell, piece) workgroups")
    ws = torch.empty(n // 4, dtype=torch.float32, device=volume.device)
    out = torch.empty_like(twists)
    _launch_polyrigid("ddrr_polyrigid_backward_twists", volume.device, volume.data_ptr(), *dims, twists.data_ptr(),
                      *grid, *h, pad, grad_out.data_ptr(), ws.data_ptr(), n, out.data_ptr())
    return out


def polyrigid_backward_volume(twists, grad_out, pitch=(1.0, 1.0, 1.0), padding="zeros"):
    """The volume gradient of :func:`polyrigid_forward`: the trilinear scatter of ``grad_out`` (float atomics: not
    bitwise reproducible on the device; ddrr_polyrigid_backward_volume) -> the volume's shape."""
    dims, grid, h, pad = _check_polyrigid("polyrigid_backward_volume", getattr(grad_out, "shape", ()), twists, pitch,
                                          padding, grad_out=grad_out)
    out = torch.empty_like(grad_out)
    _launch_polyrigid("ddrr_polyrigid_backward_volume", grad_out.device, twists.data_ptr(), *grid, *dims, *h, pad,
                      grad_out.data_ptr(), out.data_ptr())
    return out


# ------------------------------------------------- TV proximal operator (libdiffdrr_prox_hip.so)
_PROX_MODES = {"isotropic": _lib.PROX_TV_ISOTROPIC, "anisotropic": _lib.PROX_TV_ANISOTROPIC}


def _launch_prox(name, device, *args):
    """:func:`_launch` through the TV proximal operator library."""
    _launch_on(_lib.get_prox_lib(), name, device, args)


def _query_prox(name, *args):
    return _lib.get_prox_lib().query(name, *args)


def _check_prox(b, lam, spacing, mode, iterations, lower, upper, dual, x_prev, beta):
    """The domain of include/diffdrr_prox_hip.h, each condition by name -> (dims, spacing, mode code, lower,
    upper) as the entry takes them."""
    if not torch.is_tensor(b) or b.dim() != 3:
        raise ValueError("prox_tv3d: a (Dx, Dy, Dz) volume expected")
    _check_volume_like("prox_tv3d: b", b)
    if not on_device(b):
        raise ValueError("prox_tv3d: a volume on the GPU expected (prox_total_variation_3d serves the host)")
    if mode not in _PROX_MODES:
        raise ValueError(f"prox_tv3d: mode must be 'isotropic' or 'anisotropic', not {mode!r}")
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3 or not all(0.0 < s < float("inf") for s in spacing):
        raise ValueError(f"prox_tv3d: spacing must be three positive numbers, not {spacing}")
    if not 0.0 <= float(lam) < float("inf"):
        raise ValueError(f"prox_tv3d: lam must be >= 0 and finite, not {lam}")
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f"prox_tv3d: iterations must be an integer >= 0, not {iterations}")
    lo = float("-inf") if lower is None else float(lower)
    hi = float("inf") if upper is None else float(upper)
    if not lo <= hi:
        raise ValueError(f"prox_tv3d: lower {lower} must be <= upper {upper}")
    if max(b.shape) > _lib.PROX_MAX_DIM or b.numel() > 2**34:
        raise ValueError(f"prox_tv3d: at most {_lib.PROX_MAX_DIM} voxels per axis and 2^34 in all, got {tuple(b.shape)}")
    if (not torch.is_tensor(dual) or dual.dtype != torch.float32 or not dual.is_contiguous()
            or tuple(dual.shape) != (3, *b.shape) or dual.device != b.device):
        raise ValueError(f"prox_tv3d: dual must be a contiguous float32 tensor of shape {(3, *b.shape)} on {b.device}")
    if x_prev is not None:
        _check_volume_like("prox_tv3d: x_prev", x_prev, b)
        if not float("-inf") < float(beta) < float("inf"):
            raise ValueError(f"prox_tv3d: beta must be finite, not {beta}")
    return tuple(int(d) for d in b.shape), spacing, _PROX_MODES[mode], lo, hi


def prox_tv3d(b, lam, spacing=(1.0, 1.0, 1.0), mode="isotropic", iterations=20, lower=None, upper=None, dual=None,
              x_prev=None, beta=0.0):
    """``argmin_{lower <= x <= upper} 1/2 |x - b|^2 + lam TV(x)`` of a (Dx, Dy, Dz) fp32 volume on the device by
    ``iterations`` fast-gradient-projection steps from the dual start ``dual`` (3, Dx, Dy, Dz), which is updated in
    place to p_n (include/diffdrr_prox_hip.h ddrr_prox_tv3d: two passes per step, bitwise reproducible, no host
    synchronisation) -> (x, y): with ``x_prev`` the last pass also writes ``y = x + beta (x - x_prev)``, else y is
    None."""
    if dual is None:
        raise ValueError("prox_tv3d: dual is required (zeros for a cold start); it is updated in place")
    dims, spacing, code, lo, hi = _check_prox(b, lam, spacing, mode, iterations, lower, upper, dual, x_prev, beta)
    dev = b.device
    x = torch.empty_like(b)
    y = torch.empty_like(b) if x_prev is not None else None
    if b.numel() == 0:
        return x, y
    n = int(_query_prox("ddrr_prox_workspace_bytes", *dims, int(iterations))) if float(lam) > 0.0 else 0
    if n < 0:
        raise ValueError(f"prox_tv3d: no workspace for a volume of {dims}")
    scratch = torch.empty(n // 4, dtype=torch.float32, device=dev) if n else None
    _launch_prox("ddrr_prox_tv3d", dev, b.data_ptr(), *dims, *spacing, code, float(lam), int(iterations), lo, hi,
                 dual.data_ptr(), _ptr(scratch), n, x.data_ptr(), _ptr(x_prev), float(beta), _ptr(y))
    return x, y
