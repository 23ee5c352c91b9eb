// brick_shared.h -- what the translation units of the volume-stationary kernels share
// (bricks.hip: every mode on 32^3 fp32 bricks; bricks_fwd.hip: the configurable Siddon forward /
// forward + record kernel): launch arguments, the per-phase profile of tools builds, wave
// helpers, and the delivery of the float backward record.
#pragma once

#include <mutex>

#include "runtime.h"
#include "brick_core.h"
#include "brick_walk.h"
#include "record_layout.h"

namespace ddrr_brick {

using namespace ddrr;

constexpr int kQueueCap = 128;  // entries per wave and length class (63 waiting + 64 arriving)
constexpr int kBuckets = 3;     // length classes
// Float record, bricks_fwd.hip: a hit's length class is the largest estimate over its run of
// kRecordGroup adjacent lanes (8, 4, 2; 1: its own), and candidate rows start and end on multiples
// of kRecordAlign pixels (align_pixbox_rows).  Wide runs keep the lines of the record whole in one
// batch (fewer requests), narrow ones keep short hits out of long batches (fewer wave-steps).
// 4 | 4: -4.8 % instructions, +25 % requests, the step -1.0 ... -1.7 %; at 2 and 1 the requests (+47 %,
// +61 %) cost 0.15 and 0.28 ms more than the walk gains (profiles/r08/record_grouping.txt).
// The y-long bricks (32 x 64 x 32, FwdCfg::HAXIS == 1) have their own kRecordGroupY | kRecordAlignY and
// thresholds.  On views along y they have 17 % fewer hits, batches and requests at 4 | 4; spending the
// requests on 2 | 4 or 2 | 2 saves 4.5 % of the instructions as modelled and is SLOWER by 0.02 - 0.03 ms
// (requests cost time below the knee too), so 4 | 4 stays, with thresholds 26 / 56 (-0.009 ms against
// 22 / 48, four times the spread): profiles/r09/view_axis_bricks.txt.
// Tools builds choose with -DDDRR_RECORD_GROUP=n -DDDRR_RECORD_ALIGN=n (both shapes); the product has
// one value per shape.
#if defined(DDRR_EXPERIMENTS) && defined(DDRR_RECORD_GROUP)
constexpr int kRecordGroup = DDRR_RECORD_GROUP, kRecordGroupY = DDRR_RECORD_GROUP;
#else
constexpr int kRecordGroup = 4, kRecordGroupY = 4;
#endif
#if defined(DDRR_EXPERIMENTS) && defined(DDRR_RECORD_ALIGN)
constexpr int kRecordAlign = DDRR_RECORD_ALIGN, kRecordAlignY = DDRR_RECORD_ALIGN;
#else
constexpr int kRecordAlign = 4, kRecordAlignY = 4;
#endif
constexpr float kBrickT1Y = 26.f, kBrickT2Y = 56.f;  // (the z-long double bricks: 22 / 48)
constexpr bool record_width_ok(int n) { return n == 8 || n == 4 || n == 2 || n == 1; }
static_assert(record_width_ok(kRecordGroup) && record_width_ok(kRecordGroupY), "DPP maxima");
static_assert(record_width_ok(kRecordAlign) && record_width_ok(kRecordAlignY), "a power of two, at most a run of the record");

struct BrickArgs {
    const float *vol;
    Dims D;
    const float *source;  // (B, 1, 3)
    const float *target;  // (B, N, 3), row-major det_h x det_w grid
    const float *img;
    int B, det_h, det_w;
    float shift, eps;
    BrickLayout lay;
    unsigned aux_plane;  // elements per plane of the planar backward record (B * N)
    float rec_q;         // > 0: the record is the packed fixed-point form (record_pack.h), scale q
    int pix_bits;        // queue entry = (pose << pix_bits) | pixel
    float t1, t2;        // length-class thresholds on the estimated crossing count
    int dbg;             // experiment switches (tools builds with -DDDRR_EXPERIMENTS; else 0)
    int *work;           // global brick counter of this launch (zero at launch)
    const float *grad_out;  // *_VOLGRAD: dLoss/dout (B, N); BRICK_[TRI_]CHANNELS_AUX, BRICK_CHANNELS_VOLGRAD: (B, n_channels, N)
    float *g_volume;        // *_VOLGRAD: dLoss/dvolume
    int n_points;           // BRICK_TRI_*: samples per ray
    const float *amin, *amax;  // BRICK_TRI_*: device scalars (renderers.py:220-223)
    unsigned long long *prof;  // DDRR_BRICK_PROFILE builds: per-phase wave-cycle totals
    const unsigned char *labels;  // BRICK_CHANNELS: label of every voxel
    int n_channels;               // BRICK_CHANNELS: out is (B, n_channels, N)
    const float *ranges;          // 16-bit bricks: (vmin, vmax) per brick (bricks_fwd.hip)
    const int *fallback;          // ... 1: the brick is rendered from its fp32 values (q16_usable)
    int *ws_header;               // ... the workspace's header words
    int ranges_valid;             // ... already computed for this volume
    const unsigned char *packed;  // 16-bit bricks: their LDS images, brick after brick (or null)
    const unsigned *pix_mask;     // the forward kernels: bit n of word n / 32 = detector pixel n is rendered (NULL: every pixel)
    const unsigned *fingerprint;  // 16-bit bricks: bit patterns of kFingerprintWords voxels of the volume the workspace was built from
    int vec;                      // bricks_fwd.hip brick_range_kernel: 16-byte loads serve the volume
    const int *order;             // bricks_fwd.hip: k-th brick handed out (NULL: k itself)
    int *order_ws;                // ... this launch's workspace for it: order_cap weights, order_cap ints
    int order_cap;
    float *clear;                 // host side of bricks_fwd.hip: floats to zero in front of the launch (or NULL) ...
    long clear_n;                 // ... so many, by the launch that zeroes the brick counter (brick_clear_kernel);
                                  // -1: the caller has cleared them and the counter (DDRR_BRICKS_CLEARED)
    unsigned *brick_times;        // profiling builds: duration of every brick (10 ns ticks), or NULL
    int split_t, split_s;         // ... the last split_t bricks are handed out in split_s pose parts
};

// Phase timing of the brick kernel (tools/ builds with -DDDRR_BRICK_PROFILE only): s_memtime
// deltas per wave, added up per phase.  Compiled out of the product library.
#if defined(DDRR_BRICK_PROFILE)
struct BrickProf {
    unsigned long long t[16];
    unsigned long long last, born;  // born: s_memrealtime (100 MHz, one clock for all XCDs)
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = 0;
        last = __builtin_amdgcn_s_memtime();
        born = __builtin_amdgcn_s_memrealtime();
    }
    __device__ __forceinline__ void mark(int i) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        t[i] += now - last;
        last = now;
    }
    __device__ __forceinline__ void count(int i, unsigned long long n) { t[i] += n; }
};
#if defined(DDRR_TRACE_ONLY)
// (-DDDRR_TRACE_ONLY: the per-brick stage stamps of DDRR_TRACE alone -- the phase marks cost a
// scalar-memory round trip each and stretch a one-pose brick by a quarter)
#define DDRR_PROF(i)
#define DDRR_PROF_COUNT(i, n)
#define DDRR_PROF_WAIT_VMEM()
#else
#define DDRR_PROF(i) prof.mark(i)
#define DDRR_PROF_COUNT(i, n) prof.count(i, n)
#define DDRR_PROF_WAIT_VMEM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#endif
#else
struct BrickProf {};
#define DDRR_PROF(i)
#define DDRR_PROF_COUNT(i, n)
#define DDRR_PROF_WAIT_VMEM()
#endif
enum {
    PROF_STAGE = 0,   // brick id, row table, staging, barrier after it
    PROF_PULL = 1,    // unit counter, cursor, row read
    PROF_PHASE_A = 2, // candidate test, classes, queue push
    PROF_POP = 3,     // batch selection, queue read
    PROF_LOADS = 4,   // ray loads (issue + wait)
    PROF_SETUP = 5,   // exact clip, entry cell
    PROF_WALK = 6,
    PROF_DELIVER = 7, // atomics
    PROF_BARRIER = 8, // waiting for the other waves at the end of a brick
    PROF_N_BATCH = 9, PROF_N_STEPS = 10, PROF_N_UNITS = 11, PROF_N_HITS = 12,
    PROF_CLAIM = 13,   // (part of staging) brick id known
    PROF_ROWS = 14,    // (part of staging) row table written
    PROF_STORE = 15,   // (part of staging) brick stored to LDS; PROF_STAGE then is the barrier + prefix
};

// what a brick launch computes
constexpr int BRICK_FWD = 0;      // out
constexpr int BRICK_FWD_AUX = 1;  // out + planar backward record
constexpr int BRICK_VOLGRAD = 2;  // g_volume (the brick in LDS is the accumulator)
constexpr int BRICK_TRI_FWD = 3;      // trilinear marcher: out
constexpr int BRICK_TRI_VOLGRAD = 4;  // trilinear marcher: g_volume
constexpr int BRICK_TRI_FWD_AUX = 5;  // trilinear marcher: planar backward record (out follows from it)
constexpr int BRICK_CHANNELS = 6;     // out (B, C, N): one line integral per label (mask_to_channels)
constexpr int BRICK_TRI_CHANNELS = 7; // trilinear marcher, out (B, C, N): samples by the label of their nearest voxel
constexpr int BRICK_CHANNELS_AUX = 8; // backward of BRICK_CHANNELS w.r.t. the rays: the record of the volume weighted by grad_out[b, label, n]
constexpr int BRICK_TRI_CHANNELS_AUX = 9;  // backward of BRICK_TRI_CHANNELS w.r.t. the rays: the marcher's record weighted by grad_out[b, label, n]
constexpr int BRICK_CHANNELS_VOLGRAD = 10;  // backward of BRICK_CHANNELS w.r.t. the volume: the LDS accumulator's words carry the voxel's label in their low byte
constexpr int BRICK_CHANNELS_WORDS = 12;  // BRICK_CHANNELS from a volume of ready-packed words (value | label): staged like a plain brick
constexpr int BRICK_TRI_CHANNELS_VOLGRAD = 11;  // the same for the marcher (owner bricks; labels outside the owned box from the label map)


#if defined(__HIPCC__)
// v_permlane32_swap a, b: the upper 32 lanes of a change places with the lower 32 lanes of b.
// Afterwards x = a' holds a of lanes 0-31 | b of lanes 0-31, y = b' holds a of lanes 32-63 | b of
// lanes 32-63 (record_layout.h rec_halfwave_source is the host restatement).
__device__ __forceinline__ void halfwave_swap(unsigned a, unsigned b, unsigned &x, unsigned &y) {
    const auto s = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    x = s[0];
    y = s[1];
}

// The float backward record of one batch of hits, delivered to the blocked layout of
// record_layout.h.  Called by ALL lanes of the wave (ok: the lane holds a hit).  The batch's hits
// are runs of up to 8 adjacent pixels (length classes are formed per run of 8; bricks_fwd.hip: per
// run of kRecordGroup, so a run of 8 may come as two runs of 4 side by side) that start at ANY
// lane -- the class queues are compacted -- so the two 32-byte halves of a run's line, planes 0 | 1
// (2 | 3) of its rays, are brought into ONE instruction by a half-wave exchange: instruction X
// carries plane 0 (2) of the hits of lanes 0-31 in its lower half and their plane 1 (3) in its
// upper half, instruction Y the same of the hits of lanes 32-63.  2 + 2 + 1 atomic instructions,
// and only a run that straddles lanes 31 | 32 has its lines in two of them.
// v = {I, S0x, S0z, S1x, S1z}.
__device__ __forceinline__ void deliver_record_blocked(float *__restrict__ aux, bool ok,
                                                       unsigned r, const float v[5]) {
    const unsigned lo = rec_off01(r) | (ok ? 0u : 0x80000000u);  // (sign bit: nothing to add)
    unsigned xu, yu, x01u, y01u, x23u, y23u;
    halfwave_swap(lo, lo + 8u, xu, yu);
    halfwave_swap(__float_as_uint(v[0]), __float_as_uint(v[1]), x01u, y01u);
    halfwave_swap(__float_as_uint(v[2]), __float_as_uint(v[3]), x23u, y23u);
    const int xo = (int)xu, yo = (int)yu;
    const float x01 = __uint_as_float(x01u), y01 = __uint_as_float(y01u);
    const float x23 = __uint_as_float(x23u), y23 = __uint_as_float(y23u);
    if (xo >= 0) {
        unsafeAtomicAdd(aux + xo, x01);
        unsafeAtomicAdd(aux + xo + 16, x23);
    }
    if (yo >= 0) {
        unsafeAtomicAdd(aux + yo, y01);
        unsafeAtomicAdd(aux + yo + 16, y23);
    }
    if (ok) unsafeAtomicAdd(aux + rec_off4(r), v[4]);
}

// Four voxels along z from element `at` of the volume (LABELS: and their labels): one 16-byte
// load from a dword-aligned address -- global memory takes any dword alignment, and the label
// dword any alignment -- so that any D.z >= 4 is staged like a multiple of 4 (the reference's
// example CT has 133 slices).  The address is clamped to the volume's last four voxels; the one
// quad this happens to (it reaches beyond the volume's last row: none does when D.z is a multiple
// of 4) has its words shifted into place by quad_fix -- where the words are USED, so that a
// round's loads stay in flight together.  What a load picks up behind the quad's row is for the
// caller to mask.  (Volumes of fewer than four slices: brick_core.h quads_serve -- the host sends
// them to the general kernel's scalar staging.)
typedef unsigned int quad_u32x4 __attribute__((ext_vector_type(4)));  // (a native vector: plain loads / stores)
typedef unsigned int quad_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
template <bool LABELS>
__device__ __forceinline__ void quad_load(const float *__restrict__ vol,
                                          const unsigned char *__restrict__ label_map, const Dims &D,
                                          long at, quad_u32x4 &v, unsigned &labels) {
    const long a = quad_clamped_at(D, at);
    v = *reinterpret_cast<const quad_u32x4_a4 *>(vol + a);
    if (LABELS) __builtin_memcpy(&labels, label_map + a, 4);
}
// (x, y, z: the quad's first voxel; brick_core.h quad_shift says which quads were clamped.  One
// that starts behind a row's end is masked by the caller whatever it holds.)
__device__ __forceinline__ void quad_fix(const Dims &D, int x, int y, int z, quad_u32x4 &v,
                                         unsigned &labels) {
    const int shift = quad_shift(D, x, y, z);
    if (shift > 0) {
        if (shift >= 2) v = quad_u32x4{v.z, v.w, 0u, 0u};
        if (shift & 1) v = quad_u32x4{v.y, v.z, v.w, 0u};
        labels = shift < 4 ? labels >> (8 * shift) : 0u;
    }
}

__device__ __forceinline__ int lane_rank(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                          __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

#endif  // __HIPCC__

// One brick launch as its entry point describes it: the members every launch has first (an entry
// brace-initialises those, in this order), then what only some modes take, each set by name.
struct BrickLaunch {
    const float *volume;
    int dx, dy, dz;
    const float *source, *target, *img;
    int B, det_h, det_w;
    float shift, eps;
    hipStream_t st;
    void *launch_ws;  // ddrr_brick_launch_workspace_bytes
    const char *who;  // the entry's name, for its error messages
    const float *grad_out = nullptr;
    float *out = nullptr, *aux = nullptr, *g_volume = nullptr;
    int n_points = 0;
    const float *amin = nullptr, *amax = nullptr;
    float rec_q = 0.f;
    const unsigned char *labels = nullptr;
    int n_channels = 0;
    const unsigned *pix_mask = nullptr;
};

// What only the storage of the configurable forward kernel has (bricks_fwd.hip).  variant:
// DDRR_BRICKS_F32 / DDRR_BRICKS_Q16 (fp32 bricks at fewer than 8 poses, and volumes of fewer than four
// voxels, take launch_bricks).
// brick_ranges: the DDRR_BRICKS_Q16 workspace (header, (min, max) and fallback flag per brick),
// ranges_valid: it already holds this volume's.
// y_long: the 32 x 64 x 32 bricks (DDRR_BRICKS_Q16_Y / _PACKED_Y: views along y) instead of 32 x 32 x 64.
// packed: the workspace also holds the bricks' LDS images (DDRR_BRICKS_Q16_PACKED[_Y]) behind the ranges.
// clear, clear_n: floats the launch has to find zeroed (the image or the record its atomics add to):
// cleared by the launch that clears the brick counter -- one launch instead of two memsets, each
// of which is a launch of its own (5 us apiece in front of a 140 us one-pose render).
struct FwdStorage {
    int variant, packed, y_long;
    float *brick_ranges;
    int ranges_valid;
    float *clear;
    long clear_n;
};

// The kernel argument of a launch: everything zero but the launch's own description, the record's
// plane size, the queue entry's split and the experiment switches; refuses a pose batch whose ray
// indices do not fit the queue entries.  The launchers add what is theirs.
int brick_args(const BrickLaunch &l, BrickArgs &p);

// This launch's device-side state, carved out of the caller's launch workspace (bricks.hip): the
// brick counter {brick id, wmax bits, n_sum, -}, zeroed on the launch's stream, and the room for
// the hand-out order of the bricks (bricks_fwd.hip); dev, n_cu: the current device and its CU count.
long brick_launch_workspace_bytes(int dx, int dy, int dz);
int brick_launch_resources(const BrickLaunch &l, BrickArgs &p, int &dev, int &n_cu, bool zero_work = true);

// "Once per device": the state of one thing that is done at a device's first launch -- a
// function-local static of the launcher, so one per instantiation of a launcher template, i.e. per
// kernel -- and the one thing the brick launchers do that way, the raised dynamic-LDS limit.
constexpr int kMaxDev = 64;
int current_device(int &dev);  // range-checked against kMaxDev
struct OncePerDevice {
    std::mutex mu;
    bool done[kMaxDev] = {false};
};
template <class F>  // int f(): 0 or an error code (then it is tried again at the next launch)
int once_per_device(OncePerDevice &once, int dev, F f) {
    std::lock_guard<std::mutex> lock(once.mu);
    if (once.done[dev]) return 0;
    if (int rc = f()) return rc;
    once.done[dev] = true;
    return 0;
}
template <class K>
int raise_lds_limit(K *kernel, int bytes) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return e == hipSuccess ? 0 : ddrr_rt::fail_hip(e, "hipFuncSetAttribute");
}

// The 32^3 fp32 launch path of bricks.hip (every mode); bricks_fwd.hip falls back to it.
bool order_bricks(BrickArgs &q, int BX, int BY, int BZ, int nby, int nbz, int n_bricks, int slots,
                  hipStream_t st, bool zero_counter = false, int min_poses = 8);
int launch_bricks(int mode, const BrickLaunch &l);

// The configurable Siddon forward / forward + record kernel (bricks_fwd.hip).
long brick_workspace_bytes(int dx, int dy, int dz, int brick_storage);
int launch_fwd_bricks(const BrickLaunch &l, const FwdStorage &s);

// experiment switches (tools builds: mutable; product: constants)
#if defined(DDRR_EXPERIMENTS) || defined(DDRR_BRICK_PROFILE)
extern float g_brick_t1, g_brick_t2;
extern int g_brick_dbg;
extern int g_brick_variant;
extern const int *g_brick_order;
extern unsigned *g_brick_times;  // profiling builds: per-brick duration, 10 ns ticks
extern int g_brick_split_t, g_brick_split_s;
#else
constexpr float g_brick_t1 = 18.f, g_brick_t2 = 40.f;
constexpr int g_brick_dbg = 0;
#endif
#if defined(DDRR_BRICK_PROFILE)
extern unsigned long long *g_brick_prof;  // 16 device counters, see BrickProf
#endif

}  // namespace ddrr_brick
