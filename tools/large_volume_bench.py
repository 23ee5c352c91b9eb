"""Speed above 2^30 voxels: the renderer kernels at shape A = 1024 x 1024 x 1040 (1.09e9 voxels, the
64-bit per-ray walkers) against 512^3, and the 64-bit per-ray walkers against the 32-bit ones on the
same rays.

    python tools/large_volume_bench.py [--reps 20] [--out profiles/large_volume]

Writes one JSON line per case to <out>/<volume>.jsonl (512.jsonl, A.jsonl, walkers.jsonl).  Each line
holds the median kernel time of `reps` launches (HIP events around every launch) and, where bench.py
defines one, the algorithmic-bytes roofline fraction computed as bench.py computes it (SURVEY.md
section 8d): Siddon 4 B per voxel a ray visits (count_voxels) + 20 B per ray + 12 B per source, the
marcher 32 B per sample in the volume + 20 B per ray, over 8 TB/s.

The walker comparison renders a 1024^3 volume (2^30 voxels: the 32-bit instantiations) and shape A
(the Off64 ones) with the SAME rays; shape A's 16 extra z slices lie outside the field of those rays
(poses look along x and y), so both walks visit the same voxels (the lines give the counts)."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffdrr_amd import ops  # noqa: E402

HBM_PEAK_GBS = 8000.0  # as bench.py


def phantom_noise(shape, device, seed=0):
    g = torch.Generator(device).manual_seed(seed)
    vol = torch.empty(shape, dtype=torch.float32, device=device)
    c = [(d - 1) / 2 for d in shape]
    yy = ((torch.arange(shape[1], device=device) - c[1]) / (0.45 * shape[1]))[:, None] ** 2
    zz = ((torch.arange(shape[2], device=device) - c[2]) / (0.4 * shape[2]))[None, :] ** 2
    for x0 in range(0, shape[0], 64):
        x1 = min(shape[0], x0 + 64)
        xx = ((torch.arange(x0, x1, device=device) - c[0]) / (0.42 * shape[0]))[:, None, None] ** 2
        r2 = xx + yy[None] + zz[None]
        part = torch.rand((x1 - x0,) + tuple(shape[1:]), generator=g, device=device) * 0.1
        part += (r2 < 1).float() + 0.5 * (4 * r2 < 1).float()
        vol[x0:x1] = part
    return vol


def cone_rays(center, size, B, H, device, seed=0, planar=False):
    """B cone-beam poses around `center` (a DRR-like 1.6 x size source distance, a detector grid
    covering the volume); planar: directions in the x-y plane only."""
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor(center, dtype=torch.float64)
    R, W = 1.6 * size, 1.4 * size
    src, tgt = [], []
    for b in range(B):
        if planar:
            a = 2 * math.pi * b / B + 0.1
            u = torch.tensor([math.cos(a), math.sin(a), 0.0], dtype=torch.float64)
        else:
            u = torch.randn(3, generator=g, dtype=torch.float64)
            u /= u.norm()
        e1 = torch.linalg.cross(u, torch.tensor([0.3, 0.5, 0.8], dtype=torch.float64))
        e1 /= e1.norm()
        e2 = torch.linalg.cross(u, e1)
        lin = torch.linspace(-0.5, 0.5, H, dtype=torch.float64) * W
        t = (c - R * u)[None, None] + lin[:, None, None] * e1 + lin[None, :, None] * e2
        src.append((c + R * u)[None])
        tgt.append(t.reshape(-1, 3))
    s = torch.stack(src).float().to(device).contiguous()
    t = torch.stack(tgt).float().to(device).contiguous()
    return s, t, (t - s).norm(dim=-1).contiguous()


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def siddon_bytes(vol, s, t, L, H):
    nv = 0
    for a in range(0, s.shape[0], 64):
        _, _, n = ops.siddon_forward(vol, s[a:a + 64], t[a:a + 64], L[a:a + 64], count_voxels=True, det=(H, H))
        nv += int(n.sum().item())
    B = s.shape[0]
    return 4 * nv + B * H * H * 20 + 12 * B, nv


def trilinear_bytes(shape, s, t, amin, amax, P):
    D = torch.tensor(shape, device=s.device, dtype=torch.float32)
    d = t - s + 1e-8
    n_in = 0
    for m0 in range(0, P, 32):
        al = amin + (torch.arange(m0, min(P, m0 + 32), device=s.device) / (P - 1)) * (amax - amin)
        x = s[:, :, None, :] + al[None, None, :, None] * d[:, :, None, :]
        n_in += int(((x > -1) & (x < D)).all(-1).sum().item())
    return 32 * n_in + s.shape[0] * t.shape[1] * 20, n_in


def line(rows, out, **kw):
    if kw.get("alg_bytes") and kw.get("ms"):
        kw["frac"] = kw["alg_bytes"] / (kw["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
    rows.append(kw)
    print(json.dumps(kw), flush=True)
    out.write(json.dumps(kw) + "\n")
    out.flush()


def bench_volume(tag, shape, reps, outdir):
    dev = torch.device("cuda")
    vol = phantom_noise(shape, dev)
    rows = []
    H = 256
    with open(os.path.join(outdir, f"{tag}.jsonl"), "w") as out:
        center = [(d - 1) / 2 for d in shape]
        for B in (1, 32):
            s, t, L = cone_rays(center, max(shape), B, H, dev)
            alg, nv = siddon_bytes(vol, s, t, L, H)
            base = dict(volume=tag, shape=list(shape), voxels=vol.numel(), poses=B, det=[H, H])
            for storage in ("f32", "q16"):
                ms = timed(lambda: ops.siddon_forward_bricks(vol, s, t, L, (H, H), storage=storage), reps)
                line(rows, out, case="siddon_forward_bricks", storage=storage, ms=ms, alg_bytes=alg,
                     voxels_visited=nv, **base)
            ms = timed(lambda: ops.siddon_forward(vol, s, t, L, det=(H, H)), reps)
            line(rows, out, case="siddon_forward_per_ray", ms=ms, alg_bytes=alg, voxels_visited=nv, **base)
            g = torch.randn(B, H * H, device=dev)

            def fwd_bwd():
                _, aux = ops.siddon_forward_bricks(vol, s, t, L, (H, H), want_aux=True)
                ops.siddon_backward_rays(aux, g, s, t, L)
            ms = timed(fwd_bwd, reps)
            line(rows, out, case="siddon_forward_record+backward_rays (bricks, f32)", ms=ms, **base)
            ms = timed(lambda: ops.siddon_backward_volume_bricks(vol.shape, s, t, L, g, (H, H)), reps)
            line(rows, out, case="siddon_backward_volume_bricks", ms=ms, **base)
        # the marcher at 512^2
        Ht, B, P = 512, 4, 500
        s, t, L = cone_rays(center, max(shape), B, Ht, dev, seed=1)
        amin, amax = (a.reshape(1).contiguous() for a in ops.trilinear_alpha_range(s, t, vol.shape))
        alg, n_in = trilinear_bytes(shape, s, t, float(amin), float(amax), P)
        base = dict(volume=tag, shape=list(shape), voxels=vol.numel(), poses=B, det=[Ht, Ht], n_points=P)
        ms = timed(lambda: ops.trilinear_forward_bricks(vol, s, t, L, amin, amax, (Ht, Ht), n_points=P), reps)
        line(rows, out, case="trilinear_forward_bricks", ms=ms, alg_bytes=alg, samples_in_volume=n_in, **base)
        ms = timed(lambda: ops.trilinear_forward(vol, s, t, L, amin, amax, n_points=P, det=(Ht, Ht)), reps)
        line(rows, out, case="trilinear_forward_per_ray", ms=ms, alg_bytes=alg, samples_in_volume=n_in, **base)
        g = torch.randn(B, Ht * Ht, device=dev)
        ms = timed(lambda: ops.trilinear_backward_volume_bricks(vol.shape, s, t, L, g, amin, amax, (Ht, Ht),
                                                                n_points=P), reps)
        line(rows, out, case="trilinear_backward_volume_bricks", ms=ms, **base)
        ms = timed(lambda: ops.trilinear_backward(vol, s, t, L, g, amin, amax, n_points=P, det=(Ht, Ht),
                                                  want_volume=True), max(3, reps // 4))
        line(rows, out, case="trilinear_backward_per_ray (rays + volume)", ms=ms, **base)
    del vol
    torch.cuda.empty_cache()
    return rows


def bench_walkers(reps, outdir):
    """The Off64 per-ray walkers (shape A) against the 32-bit ones (1024^3) on the same rays."""
    dev = torch.device("cuda")
    shapeA, shape32 = (1024, 1024, 1040), (1024, 1024, 1024)
    H, B, P = 256, 32, 500
    # poses in the x-y plane, centred on the 1024^3 cube: the field ends below z = 1024
    s, t, L = cone_rays([511.5, 511.5, 511.5], 1024, B, H, dev, planar=True)
    g = torch.randn(B, H * H, device=dev)
    rows = []
    with open(os.path.join(outdir, "walkers.jsonl"), "w") as out:
        for tag, shape in (("32-bit, 1024^3", shape32), ("Off64, 1024x1024x1040", shapeA)):
            vol = phantom_noise(shape, dev)
            alg, nv = siddon_bytes(vol, s, t, L, H)
            amin, amax = (a.reshape(1).contiguous() for a in ops.trilinear_alpha_range(s, t, shape32))
            base = dict(walker=tag, shape=list(shape), poses=B, det=[H, H], voxels_visited=nv)
            ms = timed(lambda: ops.siddon_forward(vol, s, t, L, det=(H, H)), reps)
            line(rows, out, case="siddon_forward_per_ray", ms=ms, alg_bytes=alg, ns_per_voxel=ms * 1e6 / nv, **base)
            ms = timed(lambda: ops.siddon_forward(vol, s, t, L, det=(H, H), want_aux=True), reps)
            line(rows, out, case="siddon_forward_per_ray (record)", ms=ms, **base)
            ms = timed(lambda: ops.siddon_backward_volume(vol, s, t, L, g, det=(H, H)), max(3, reps // 4))
            line(rows, out, case="siddon_backward_volume (per-ray scatter)", ms=ms, **base)
            ms = timed(lambda: ops.trilinear_forward(vol, s, t, L, amin, amax, n_points=P, det=(H, H)), reps)
            line(rows, out, case="trilinear_forward_per_ray", ms=ms, n_points=P, **base)
            del vol
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "large_volume"))
    ap.add_argument("--only", choices=["512", "A", "walkers"], default=None)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.only in (None, "512"):
        bench_volume("512", (512, 512, 512), a.reps, a.out)
    if a.only in (None, "A"):
        bench_volume("A", (1024, 1024, 1040), a.reps, a.out)
    if a.only in (None, "walkers"):
        bench_walkers(a.reps, a.out)


if __name__ == "__main__":
    main()
