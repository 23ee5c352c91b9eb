"""CPU model of the bookkeeping of the forward + record brick kernel (csrc/bricks_fwd.hip, the
32 x 32 x 64 16-bit bricks of the headline) and of what its record delivery asks of the memory
side: one REQUEST per 64-byte line touched by one atomic instruction (tools/ubench/atomic_merge.hip:
the lanes of one instruction are merged per line wherever in the wave they sit, two instructions
never are).  Nothing here runs on a GPU.

Modelled, for the poses and the detector of ``bench.py`` (``bench.perturbed_poses``):
  * project_brick_grid, align_pixbox_rows, brick_row and brick_candidate (csrc/brick_walk.h) in
    float32, candidate by candidate;
  * the length classes per run of ``--group`` adjacent lanes (csrc/brick_shared.h kRecordGroup) at the
    thresholds ``--t1`` / ``--t2`` (22 / 48: what bricks_fwd.hip hands the 16-bit bricks), candidate rows
    aligned to ``--align`` pixels (kRecordAlign);
  * the walk: a batch takes as many wave-steps as its longest hit, estimated as n_est + 2; the live-lane
    fraction is the hits' own crossings (n_est) over 64 lanes times the batches' steps;
  * the per-wave class queues (128 entries, compacted by lane rank, popped 64 from the top);
  * the pooled end of a brick (segments longest class first, cut into batches of 64);
  * the delivery, lane by lane: ``delivery_lanes`` is the restatement of
    csrc/brick_shared.h deliver_record_blocked that tests/test_record_delivery_model.py checks.
Which wave pulls which unit is decided by an LDS counter at run time; the model hands the units out
to the wave that has walked the fewest batches (ties: lowest wave), which is what equal walks give.
Every candidate that passes phase A counts as a hit (the kernel drops the few whose exact clip
misses the brick; counters against the model: profiles/r07/record_delivery.txt).

    python tools/record_requests.py [--poses 32] [--every 17] [--group 4] [--align 4] [--t1 22] [--t2 48]
                                    [--brick 32,32,64]
prints units, hits, batches, wave-steps, the live-lane fraction, runs, the full-run fraction and the
requests per launch of every delivery form, sampled over every ``--every``-th brick and scaled to all
of them (profiles/r08/record_grouping.txt: the widths against the counters).  The defaults are the
product's z-long bricks'; ``--group 8 --align 8`` is the kernel of profiles/r07/record_delivery.txt;
``--brick 32,64,32 --t1 26 --t2 56`` the y-long configuration (profiles/r09/view_axis_bricks.txt).
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
REC_BLOCK_FLOATS = 80
QUEUE_CAP, WAVES, T1, T2 = 128, 16, 22.0, 48.0  # (bricks_fwd.hip launch_fwd_bricks: the 16-bit storages)
BRICK = (32, 32, 64)
MARGIN, SHIFT, EPS = F(0.01), F(0.5), F(1e-8)


# ----------------------------------------------------------------- the record's layout

def rec_off01(r):
    """csrc/record_layout.h rec_off01: float index of plane 0 of ray r (plane 1: + 8, planes 2 | 3: + 16)."""
    return (r >> 4) * REC_BLOCK_FLOATS + ((r >> 3) & 1) * 32 + (r & 7)


def rec_off4(r):
    return (r >> 4) * REC_BLOCK_FLOATS + 64 + (r & 15)


def rec_index(r, plane):
    """csrc/record_layout.h rec_index"""
    blk = (r >> 4) * REC_BLOCK_FLOATS
    if plane == 4:
        return blk + 64 + (r & 15)
    return blk + ((r >> 3) & 1) * 32 + (plane >> 1) * 16 + (plane & 1) * 8 + (r & 7)


# ----------------------------------------------------------------- the delivery, lane by lane

FORMS = ("row_xor8", "half_wave")


def delivery_lanes(rays, form="half_wave"):
    """The atomic instructions that deliver one batch.  rays: the ray index the batch holds in
    lane 0, 1, ... (at most 64; -1: the lane holds no hit; lanes behind the list hold none).
    -> five lists, one per instruction in issue order (X planes 0 | 1, X planes 2 | 3, Y planes
    0 | 1, Y planes 2 | 3, plane 4), of (lane, float index, source lane, plane): `lane` adds plane
    `plane` of the hit that `source lane` holds at `float index` of the record.

    "half_wave" (csrc/brick_shared.h deliver_record_blocked, record_layout.h rec_halfwave_source):
    X carries the hits of lanes 0-31 -- plane 0 (2) in its lower half, plane 1 (3) in its upper
    half --, Y the hits of lanes 32-63.  "row_xor8": the delivery up to round 6, lane l exchanges
    with lane l ^ 8."""
    ray = np.full(64, -1, dtype=np.int64)
    ray[:len(rays)] = rays
    out = [[], [], [], [], []]
    for instr in (0, 1):  # X, Y
        for lane in range(64):
            if form == "half_wave":
                upper, src = lane >> 5, (lane & 31) + 32 * instr
            elif form == "row_xor8":
                upper = (lane >> 3) & 1  # lanes 0-7 of a row: plane 0 (2), lanes 8-15: plane 1 (3)
                src = lane if upper == instr else lane ^ 8  # X: lanes 0-7 their own hit, Y: lanes 8-15
            else:
                raise ValueError(form)
            if ray[src] < 0:  # (the sign bit of the offset travels with it: nothing to add)
                continue
            at = rec_off01(int(ray[src])) + 8 * upper
            out[2 * instr].append((lane, at, src, upper))
            out[2 * instr + 1].append((lane, at + 16, src, 2 + upper))
    for lane in range(64):
        if ray[lane] >= 0:
            out[4].append((lane, rec_off4(int(ray[lane])), lane, 4))
    return out


def batch_requests(rays, form):
    """64-byte lines touched, summed over the batch's instructions."""
    ray = np.full(64, -1, dtype=np.int64)
    ray[:len(rays)] = rays
    ok = ray >= 0
    o0 = rec_off01(np.where(ok, ray, 0))
    lane = np.arange(64)
    n = 0
    for instr in (0, 1):
        if form == "half_wave":
            upper, src = lane >> 5, (lane & 31) + 32 * instr
        else:
            upper = (lane >> 3) & 1
            src = np.where(upper == instr, lane, lane ^ 8)
        at = (o0[src] + 8 * upper)[ok[src]]
        n += 2 * len(np.unique(at >> 4))  # (planes 2 | 3: the same lines + 1)
    return n + len(np.unique(rec_off4(ray[ok]) >> 4))


# ----------------------------------------------------------------- phase A (csrc/brick_walk.h)

def pose_grid(src, tgt, H, W):
    t = tgt.reshape(H, W, 3)
    return dict(s=src.astype(F), t00=t[0, 0].astype(F),
                ei=((t[H - 1, 0] - t[0, 0]).astype(F) * (F(1) / F(H - 1))).astype(F),
                ej=((t[0, W - 1] - t[0, 0]).astype(F) * (F(1) / F(W - 1))).astype(F))


def project_brick_grid(g, H, W, lo, hi):
    r = (g["t00"] - g["s"]).astype(F)
    ei, ej = g["ei"], g["ej"]
    n = np.cross(ei, ej).astype(F)
    rxej, rxei = np.cross(r, ej).astype(F), np.cross(r, ei).astype(F)
    c = np.arange(8)
    w = np.stack([np.where(c & (1 << a), hi[a], lo[a]).astype(F) - SHIFT - g["s"][a] for a in range(3)], 1).astype(F)
    det = (w @ n).astype(F)
    if not ((det > 0).all() or (det < 0).all()):
        return 0, H - 1, 0, W - 1
    with np.errstate(all="ignore"):
        i = (-(w @ rxej) / det).astype(F)
        j = ((w @ rxei) / det).astype(F)
    gb = F(0.02)
    fi0, fi1 = max(math.floor(i.min() - gb), 0), min(math.ceil(i.max() + gb), H - 1)
    fj0, fj1 = max(math.floor(j.min() - gb), 0), min(math.ceil(j.max() + gb), W - 1)
    if not (fi0 <= fi1) or not (fj0 <= fj1):
        return 0, -1, 0, -1
    return int(fi0), int(fi1), int(fj0), int(fj1)


def align_pixbox_rows(pb, W, align=8):
    i0, i1, j0, j1 = pb
    if j1 < j0 or i1 < i0:
        return pb
    m = align - 1
    return i0, i1, j0 & ~m, min(j1 | m, W - 1)


def brick_candidates(g, pb, lo, hi, W):
    """-> (pix, hit, n_est) of every candidate of the pixel box, row-major (brick_candidate)."""
    i0, i1, j0, j1 = pb
    if j1 < j0 or i1 < i0:
        z = np.zeros(0)
        return z.astype(np.int64), z.astype(bool), z.astype(F)
    ii, jj = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1), indexing="ij")
    fi, fj = ii.ravel().astype(F), jj.ravel().astype(F)
    entry, exit_, l1 = np.full(fi.shape, -np.inf, F), np.full(fi.shape, np.inf, F), np.zeros(fi.shape, F)
    with np.errstate(all="ignore"):
        for a in range(3):
            D0 = F(F(g["t00"][a] - g["s"][a]) + EPS)
            P0 = F(F(F(lo[a]) - MARGIN) - SHIFT) - g["s"][a]
            P1 = F(F(F(hi[a]) + MARGIN) - SHIFT) - g["s"][a]
            d = (fj * g["ej"][a] + (fi * g["ei"][a] + D0)).astype(F)
            inv = (F(1) / d).astype(F)
            a0, a1 = (F(P0) * inv).astype(F), (F(P1) * inv).astype(F)
            entry = np.maximum(entry, np.minimum(a0, a1))
            exit_ = np.minimum(exit_, np.maximum(a0, a1))
            l1 = l1 + np.abs(d)
        n_est = ((exit_ - entry) * l1).astype(F)
    return ii.ravel() * W + jj.ravel(), entry < exit_, n_est


# ----------------------------------------------------------------- queues, pool, batches

def cut_on_runs(L):
    """Step 4 of the delivery's accounting, modelled only: a batch that neither ends inside a run
    of 8 nor has one across lanes 31 | 32.  L: queue entries from the side they are taken from.
    -> (the batch's 64 lanes, -1 where a lane stays empty; entries taken)."""
    m = min(len(L), 65)
    bounds = [i for i in range(1, m) if L[i] >> 3 != L[i - 1] >> 3] + ([len(L)] if len(L) <= 64 else [])
    b = max(i for i in bounds if i <= 32)
    e = max(i for i in bounds if i - b <= 32)
    lanes = [-1] * 64
    lanes[:b] = L[:b]
    lanes[32:32 + e - b] = L[b:e]
    return lanes, e


def brick_batches(units, cut=False, group=8, t1=T1, t2=T2):
    """units: per unit of 64 candidates, (ray index, hit, n_est) arrays of at most 64 lanes.
    cut: batches end on run boundaries and have one at lanes 31 | 32 (cut_on_runs).
    group: lanes per run that share a length class (the largest n_est of the run's hits).
    -> (batches: lists of ray indices in lane order, runs, full runs, hits)."""
    queues = [[[] for _ in range(3)] for _ in range(WAVES)]
    walked = [0] * WAVES
    batches, runs, full, hits = [], 0, 0, 0
    for ray, hit, n_est in units:
        wv = min(range(WAVES), key=lambda k: (walked[k], k))
        m = len(ray)
        n = np.zeros(64, F)
        n[:m] = np.where(hit, n_est, F(0))
        grp = np.repeat(n.reshape(64 // group, group).max(1), group)[:m]  # classes per run of `group` lanes
        per_run = np.add.reduceat(hit.astype(np.int64), np.arange(0, m, 8))
        runs += int((per_run > 0).sum())
        full += int((per_run == 8).sum())
        hits += int(hit.sum())
        cls = np.where(grp < t1, 0, np.where(grp < t2, 1, 2))
        for k in range(3):
            queues[wv][k].extend(ray[hit & (cls == k)].tolist())  # (lane_rank: compacted, lane order)
        walked[wv] += 1
        while True:
            k = next((k for k in range(3) if len(queues[wv][k]) >= 64), -1)
            if k < 0:
                break
            q = queues[wv][k]
            assert len(q) < QUEUE_CAP
            if cut:
                lanes, e = cut_on_runs(q[::-1][:65])
                batches.append(lanes)
                del q[-e:]
            else:
                batches.append(q[-64:])
                del q[-64:]
            walked[wv] += 4
    # the pool: segments (class 2, wave 0 .. 15), (class 1, ...), (class 0, ...), cut into 64s
    pooled = [e for k in (2, 1, 0) for wv in range(WAVES) for e in queues[wv][k]]
    if cut:
        j = 0
        while j < len(pooled):
            lanes, e = cut_on_runs(pooled[j:j + 65])
            batches.append(lanes)
            j += e
    else:
        batches += [pooled[j:j + 64] for j in range(0, len(pooled), 64)]
    return batches, runs, full, hits


def bench_rays(B, D=512, H=256):
    """Voxel-space sources (B, 3) and targets (B, H * H, 3) of bench.py's headline poses."""
    import torch

    import bench
    from diffdrr_amd import DRR
    from diffdrr_amd.data import make_subject
    from diffdrr_amd.pose import convert

    subject = make_subject(torch.zeros(D, D, D), spacing=(1.0, 1.0, 1.0), orientation="AP")
    drr = DRR(subject, sdd=1020.0, height=H, delx=2.4 * (256 / H) * (D / 512), renderer="siddon")
    rot, xyz = bench.perturbed_poses(B, seed=2, device="cpu")
    with torch.no_grad():
        pose = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
        s, t = drr.detector(pose, None)
        s, t = drr.affine_inverse(s), drr.affine_inverse(t)
    return s.reshape(B, 3).numpy().astype(F), t.reshape(B, H * H, 3).numpy().astype(F)


def walk_steps(batches, steps_of):
    """-> (wave-steps of the batches: each walks as long as its longest hit; the hits' own crossings).
    steps_of: ray index -> estimated steps of the hit (n_est + 2: entry, exit and rounding)."""
    wave, own = 0.0, 0.0
    for bt in batches:
        st = [steps_of[r] for r in bt if r >= 0]
        wave += max(st)
        own += sum(st) - 2.0 * len(st)
    return wave, own


def model(src, tgt, dims, H, W, every=17, forms=FORMS, group=8, align=8, t1=T1, t2=T2, brick=BRICK):
    """brick: the bricks' extent (BX, BY, BZ) -- 32 x 32 x 64, or 32 x 64 x 32 (the y-long configuration)."""
    BRICK = tuple(brick)  # noqa: N806 (shadows the module's default on purpose)
    B = src.shape[0]
    grids = [pose_grid(src[b], tgt[b], H, W) for b in range(B)]
    nb = [-(-dims[a] // BRICK[a]) for a in range(3)]
    n_bricks = nb[0] * nb[1] * nb[2]
    tot = dict(hits=0, batches=0, runs=0, full=0, cut_batches=0, half_wave_cut=0, units=0, wave_steps=0.0,
               own_steps=0.0, **{f: 0 for f in forms})
    sampled = 0
    for brick in range(every // 2, n_bricks, every):
        bz, by, bx = brick % nb[2], (brick // nb[2]) % nb[1], brick // (nb[2] * nb[1])
        lo = [bx * BRICK[0], by * BRICK[1], bz * BRICK[2]]
        hi = [min(lo[a] + BRICK[a], dims[a]) for a in range(3)]
        units, steps_of = [], {}
        for b in range(B):  # (B <= 32: one chunk)
            pb = align_pixbox_rows(project_brick_grid(grids[b], H, W, lo, hi), W, align)
            pix, hit, n_est = brick_candidates(grids[b], pb, lo, hi, W)
            ray = b * H * W + pix
            units += [(ray[k:k + 64], hit[k:k + 64], n_est[k:k + 64]) for k in range(0, len(ray), 64)]
            steps_of.update(zip(ray[hit].tolist(), (n_est[hit] + F(2)).tolist()))
        batches, runs, full, hits = brick_batches(units, group=group, t1=t1, t2=t2)
        wave, own = walk_steps(batches, steps_of)
        tot["units"] += len(units)
        tot["wave_steps"] += wave
        tot["own_steps"] += own
        tot["hits"] += hits
        tot["batches"] += len(batches)
        tot["runs"] += runs
        tot["full"] += full
        for f in forms:
            tot[f] += sum(batch_requests(np.asarray(bt, dtype=np.int64), f) for bt in batches)
        cut = brick_batches(units, cut=True, group=group, t1=t1, t2=t2)[0]
        tot["cut_batches"] += len(cut)
        tot["half_wave_cut"] += sum(batch_requests(np.asarray(bt, dtype=np.int64), "half_wave") for bt in cut)
        sampled += 1
    scale = n_bricks / sampled
    res = {k: v * scale for k, v in tot.items()}
    res["full_fraction"] = tot["full"] / max(tot["runs"], 1)
    res["live_lanes"] = tot["own_steps"] / max(64.0 * tot["wave_steps"], 1.0)
    res["floor"] = 2.5 * res["runs"]
    res["sampled_bricks"], res["bricks"] = sampled, n_bricks
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--poses", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--det", type=int, default=256)
    ap.add_argument("--every", type=int, default=17, help="model every n-th brick (odd: every brick row, column and layer is met)")
    ap.add_argument("--group", type=int, default=4, choices=[8, 4, 2, 1], help="lanes per run that share a length class")
    ap.add_argument("--align", type=int, default=4, choices=[8, 4, 2, 1], help="candidate rows start and end on multiples of this")
    ap.add_argument("--t1", type=float, default=T1, help="length-class thresholds on n_est, as the kernel sees them")
    ap.add_argument("--t2", type=float, default=T2)
    ap.add_argument("--brick", default=",".join(map(str, BRICK)), help="the bricks' extent BX,BY,BZ (32,64,32: y-long)")
    a = ap.parse_args()
    src, tgt = bench_rays(a.poses, a.size, a.det)
    brick = tuple(int(v) for v in a.brick.split(","))
    if len(brick) != 3 or min(brick) < 1:
        ap.error("--brick BX,BY,BZ")
    r = model(src, tgt, (a.size,) * 3, a.det, a.det, a.every, group=a.group, align=a.align, t1=a.t1, t2=a.t2,
              brick=brick)
    print(f"{a.size}^3 -> {a.det}^2, {a.poses} poses, {r['sampled_bricks']} of {r['bricks']} bricks "
          f"({brick[0]} x {brick[1]} x {brick[2]}) modelled; "
          f"classes per run of {a.group}, rows aligned to {a.align}, thresholds {a.t1:g} / {a.t2:g}; per launch:")
    print(f"  units                {r['units']:.3e}")
    print(f"  hits                 {r['hits']:.3e}")
    print(f"  batches              {r['batches']:.3e}")
    print(f"  wave-steps           {r['wave_steps']:.3e}  (live lanes: {r['live_lanes']:.3f})")
    print(f"  runs                 {r['runs']:.3e}  (full: {100 * r['full_fraction']:.1f} %, "
          f"{r['hits'] / r['runs']:.2f} hits per run)")
    print(f"  requests, lane ^ 8 exchange (up to round 6)   {r['row_xor8']:.4e}  "
          f"({8 * r['row_xor8'] / r['hits']:.2f} per 8 hits)")
    print(f"  requests, half-wave exchange (built)          {r['half_wave']:.4e}  "
          f"({8 * r['half_wave'] / r['hits']:.2f} per 8 hits, {100 * (r['half_wave'] / r['row_xor8'] - 1):+.1f} %)")
    print(f"  requests, half-wave + batches cut on runs     {r['half_wave_cut']:.4e}  "
          f"({100 * (r['half_wave_cut'] / r['half_wave'] - 1):+.1f} % requests for "
          f"{100 * (r['cut_batches'] / r['batches'] - 1):+.1f} % batches: modelled, not built)")
    print(f"  requests, floor of the layout (2.5 per run)   {r['floor']:.4e}")


if __name__ == "__main__":
    main()
