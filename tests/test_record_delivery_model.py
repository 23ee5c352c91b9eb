"""The lane mapping of the record delivery as tools/record_requests.py restates it
(delivery_lanes; the kernel: csrc/brick_shared.h deliver_record_blocked, the host restatement of
its exchange: csrc/record_layout.h rec_halfwave_source): whatever runs a batch holds and at
whatever lane they start, every (hit, plane) is added exactly once, at rec_index(ray, plane), and
a lane without a hit adds nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import record_requests as rr  # noqa: E402


def random_batch(rng, n, n_rays, holes=False):
    """n lanes of runs of 1 .. 8 adjacent rays inside one group of 8, starting at any lane; the
    rays of a batch are distinct (an entry is one (ray, brick) pair).  holes: some lanes hold no hit
    (a candidate whose exact clip misses the brick)."""
    groups = rng.permutation((n_rays + 7) // 8)
    rays = []
    for g in groups:
        if len(rays) >= n:
            break
        lo = int(rng.integers(0, 8))
        ln = int(rng.integers(1, 9 - lo))
        run = [8 * int(g) + lo + k for k in range(ln) if 8 * int(g) + lo + k < n_rays]
        rays += run[:n - len(rays)]
    rays = np.asarray(rays, dtype=np.int64)
    if holes:
        rays = np.where(rng.random(len(rays)) < 0.2, -1, rays)
    return rays


def check(rays, n_rays, form="half_wave"):
    instrs = rr.delivery_lanes(rays, form)
    assert len(instrs) == 5
    record = np.zeros((rr.rec_index(n_rays - 1, 4) // rr.REC_BLOCK_FLOATS + 1) * rr.REC_BLOCK_FLOATS, dtype=np.int64)
    seen = set()
    for ins in instrs:
        lanes = [lane for lane, _, _, _ in ins]
        assert len(set(lanes)) == len(lanes) and all(0 <= lane < 64 for lane in lanes)  # one add per lane
        for lane, at, src, plane in ins:
            assert 0 <= src < len(rays) and rays[src] >= 0, "a lane without a hit adds nothing"
            assert at == rr.rec_index(int(rays[src]), plane), (lane, src, plane)
            assert (src, plane) not in seen, "added twice"
            seen.add((src, plane))
            record[at] += 1
    hits = [k for k in range(len(rays)) if rays[k] >= 0]
    assert seen == {(k, p) for k in hits for p in range(5)}
    # the record holds one add at each (ray, plane) of the batch and nothing elsewhere
    want = np.zeros_like(record)
    for k in hits:
        for p in range(5):
            want[rr.rec_index(int(rays[k]), p)] += 1
    assert np.array_equal(record, want) and record.max(initial=0) <= 1
    return instrs


@pytest.mark.parametrize("form", rr.FORMS)
def test_random_batches_add_every_plane_once(form):
    rng = np.random.default_rng(0)
    for n in list(range(1, 65)) * 3:
        for n_rays in (3 * 19 * 21, 35, 4096):  # (1197 and 35: no multiples of 16 -- the last block is partial)
            rays = random_batch(rng, n, n_rays, holes=bool(n & 1))
            check(rays, n_rays, form)


def test_fewer_than_32_entries_leave_y_empty():
    rng = np.random.default_rng(1)
    for n in (1, 7, 8, 31, 32):
        x01, x23, y01, y23, p4 = check(random_batch(rng, n, 4096), 4096)
        assert y01 == [] and y23 == []
        assert len(x01) == 2 * n and len(x23) == 2 * n and len(p4) == n


def test_33_entries():
    rng = np.random.default_rng(2)
    rays = random_batch(rng, 33, 1197)
    assert len(rays) == 33
    x01, x23, y01, y23, p4 = check(rays, 1197)
    # Y carries the one hit of lane 32: its plane 0 in lane 0, its plane 1 in lane 32
    assert sorted((lane, src, plane) for lane, _, src, plane in y01) == [(0, 32, 0), (32, 32, 1)]
    assert sorted((lane, src, plane) for lane, _, src, plane in y23) == [(0, 32, 2), (32, 32, 3)]


def test_run_across_lanes_31_and_32():
    # 28 lanes of other runs, then one full run of 8 in lanes 28 .. 35
    rays = np.concatenate([np.arange(0, 28), np.arange(160, 168), np.arange(320, 340)])
    x01, _, y01, _, _ = check(rays, 1197)
    line = lambda at: at >> 4  # noqa: E731
    in_x = {line(at) for _, at, src, _ in x01 if 28 <= src < 36}
    in_y = {line(at) for _, at, src, _ in y01 if 28 <= src < 36}
    assert in_x == in_y and len(in_x) == 1  # the run's line of planes 0 | 1 is requested by X and by Y
    # while a run inside one half has both halves of its line in one instruction: one request
    assert rr.batch_requests(np.arange(160, 168), "half_wave") == 3
    assert rr.batch_requests(np.arange(160, 168), "row_xor8") == 3  # (on an 8-lane boundary the old form too)
    off = np.concatenate([np.arange(3), np.arange(160, 168)])  # the same run from lane 3 on
    assert rr.batch_requests(off, "half_wave") == 6 and rr.batch_requests(off, "row_xor8") == 8


def test_partial_last_block():
    # 35 rays: block 2 holds rays 32 .. 34 only; every add stays inside the record's 3 blocks
    rays = np.arange(35)
    for form in rr.FORMS:
        instrs = check(rays, 35, form)
        assert max(at for ins in instrs for _, at, _, _ in ins) < 3 * rr.REC_BLOCK_FLOATS


def test_layout_restatement_matches_the_header():
    """rec_off01 / rec_off4 / rec_index of the tool against csrc/record_layout.h's formulas, read
    from the header's text (the GPU tests hold the kernel to the same layout through
    ops.record_planes)."""
    header = open(os.path.join(rr.ROOT, "diffdrr_amd", "csrc", "record_layout.h")).read()
    assert "(r >> 4) * (unsigned)kRecBlockFloats + ((r >> 3) & 1u) * 32u + (r & 7u)" in header
    assert "(r >> 4) * (unsigned)kRecBlockFloats + 64u + (r & 15u)" in header
    assert "upper = lane >> 5;" in header and "src = (lane & 31) + 32 * instr;" in header
    for r in (0, 7, 8, 15, 16, 1196):
        assert rr.rec_index(r, 0) == rr.rec_off01(r) and rr.rec_index(r, 1) == rr.rec_off01(r) + 8
        assert rr.rec_index(r, 2) == rr.rec_off01(r) + 16 and rr.rec_index(r, 3) == rr.rec_off01(r) + 24
        assert rr.rec_index(r, 4) == rr.rec_off4(r)
