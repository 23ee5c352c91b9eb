// Host build of csrc/prox_core.h behind the C ABI of include/diffdrr_prox_hip.h: the passes of the gfx950 kernels
// (csrc/prox.hip) as plain loops over the voxels, each voxel through the same functions with the same selects.
// No sum crosses a voxel, so the order of the loops is immaterial.  Compiled by tests/prox_cases.py with g++; no
// HIP, no GPU.  Pointers are host pointers; `stream` is ignored.  With -DPROX_EMU_MAIN it is a program of its own
// that runs the entry on exactly-sized heap buffers (built with -fsanitize=address,undefined: the memory check of
// the index arithmetic).
#include <stdio.h>

#include <vector>

#include "../../diffdrr_amd/csrc/prox_core.h"

namespace {

using namespace ddrr_prox;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

// prox_primal_kernel: r NULL = no dual term; x_prev / y the epilogue
void primal_pass(const Params &q, const float *b, const float *r, float *x, const float *x_prev, float beta, float *y) {
    const long n = (long)q.Dx * q.Dy * q.Dz, sj = q.Dz, si = (long)q.Dy * q.Dz;
    for (int i = 0; i < q.Dx; ++i)
        for (int j = 0; j < q.Dy; ++j)
            for (int k = 0; k < q.Dz; ++k) {
                const long at = i * si + j * sj + k;
                float u[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (r) {
                    u[0] = i + 1 < q.Dx ? r[at] : 0.f;
                    u[1] = i > 0 ? r[at - si] : 0.f;
                    u[2] = j + 1 < q.Dy ? r[n + at] : 0.f;
                    u[3] = j > 0 ? r[n + at - sj] : 0.f;
                    u[4] = k + 1 < q.Dz ? r[2 * n + at] : 0.f;
                    u[5] = k > 0 ? r[2 * n + at - 1] : 0.f;
                }
                const float v = primal(b[at], u[0], u[1], u[2], u[3], u[4], u[5], q);
                const float prev = x_prev ? x_prev[at] : 0.f;  // (y may be x_prev itself)
                x[at] = v;
                if (x_prev) y[at] = extrapolate(v, prev, beta);
            }
}

// prox_dual_kernel
template <int MODE>
void dual_pass(const Params &q, const float *x, const float *r_in, float *p, float *r_out, float c) {
    const long n = (long)q.Dx * q.Dy * q.Dz, sj = q.Dz, si = (long)q.Dy * q.Dz;
    for (int i = 0; i < q.Dx; ++i)
        for (int j = 0; j < q.Dy; ++j)
            for (int k = 0; k < q.Dz; ++k) {
                const long at = i * si + j * sj + k;
                const bool okx = i + 1 < q.Dx, oky = j + 1 < q.Dy, okz = k + 1 < q.Dz;
                const float d[3] = {difference(x[at], x[okx ? at + si : at], q.isx, okx),
                                    difference(x[at], x[oky ? at + sj : at], q.isy, oky),
                                    difference(x[at], x[okz ? at + 1 : at], q.isz, okz)};
                float pv[3] = {p[at], p[n + at], p[2 * n + at]}, rv[3] = {r_in[at], r_in[n + at], r_in[2 * n + at]};
                dual_step<MODE>(d, q.inv, c, pv, rv);
                for (int a = 0; a < 3; ++a) {
                    p[a * n + at] = pv[a];
                    if (r_out) r_out[a * n + at] = rv[a];
                }
            }
}

}  // namespace

extern "C" {

int ddrr_prox_abi_version(void) { return DDRR_PROX_ABI_VERSION; }
const char *ddrr_prox_last_error(void) { return g_err; }

long ddrr_prox_workspace_bytes(int Dx, int Dy, int Dz, int iterations) {
    if (const char *what = dims_error(Dx, Dy, Dz)) return fail(-1, what);
    if (iterations < 0) return fail(-1, "iterations must be >= 0");
    return workspace_bytes(Dx, Dy, Dz, iterations);
}

int ddrr_prox_tv3d(const float *b, int Dx, int Dy, int Dz, float sx, float sy, float sz, int mode, float lambda,
                   int iterations, float lower, float upper, float *dual, float *scratch, long scratch_bytes,
                   float *x_out, const float *x_prev, float beta, float *y_out, void *) {
    if (const char *what = argument_error(b, Dx, Dy, Dz, sx, sy, sz, mode, lambda, iterations, lower, upper, dual,
                                          scratch, scratch_bytes, x_out, x_prev, beta, y_out))
        return fail(-1, what);
    if ((long)Dx * Dy * Dz == 0) return 0;
    const Params q = make_params(Dx, Dy, Dz, sx, sy, sz, lambda, lower, upper);
    double t = 1.0;
    for (int k = 0; lambda > 0.f && k < iterations; ++k) {
        const float *r_in = k == 0 ? dual : scratch;
        primal_pass(q, b, r_in, x_out, nullptr, 0.f, nullptr);
        const double t1 = next_t(t);
        const float c = (float)((t - 1.0) / t1);
        float *r_out = k + 1 < iterations ? scratch : nullptr;
        t = t1;
        if (mode == DDRR_PROX_TV_ISOTROPIC)
            dual_pass<DDRR_PROX_TV_ISOTROPIC>(q, x_out, r_in, dual, r_out, c);
        else
            dual_pass<DDRR_PROX_TV_ANISOTROPIC>(q, x_out, r_in, dual, r_out, c);
    }
    primal_pass(q, b, lambda > 0.f ? dual : nullptr, x_out, x_prev, beta, y_out);
    return 0;
}

}  // extern "C"

#ifdef PROX_EMU_MAIN
namespace {

unsigned g_seed = 12345u;

float uniform() {  // in [0, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) / 16777216.f;
}

int run(int Dx, int Dy, int Dz, int mode, int iterations, bool epilogue) {
    const size_t n = (size_t)Dx * Dy * Dz;
    std::vector<float> b(n), dual(3 * n, 0.f), x(n), xp(n), y(n);
    for (float &v : b) v = uniform();
    for (float &v : xp) v = uniform();
    const long bytes = ddrr_prox_workspace_bytes(Dx, Dy, Dz, iterations);
    if (bytes < 0) return 1;
    std::vector<float> scratch((size_t)bytes / 4);
    const int rc = ddrr_prox_tv3d(b.data(), Dx, Dy, Dz, 0.8f, 1.7f, 2.5f, mode, 0.05f, iterations, 0.2f, 0.9f,
                                  dual.data(), bytes ? scratch.data() : nullptr, bytes, x.data(),
                                  epilogue ? xp.data() : nullptr, 0.7f, epilogue ? y.data() : nullptr, nullptr);
    double sx = 0, sp = 0;
    for (float v : x) sx += v;
    for (float v : dual) sp += v;
    printf("%dx%dx%d mode %d, %d iterations: rc %d, sums %.6g %.6g\n", Dx, Dy, Dz, mode, iterations, rc, sx, sp);
    return rc;
}

}  // namespace

int main() {
    int rc = 0;
    for (int mode = 0; mode < 2; ++mode) {
        rc |= run(1, 1, 7, mode, 3, false);
        rc |= run(2, 3, 4, mode, 0, true);
        rc |= run(5, 70, 9, mode, 3, true);
        rc |= run(33, 17, 67, mode, 2, true);
    }
    return rc;
}
#endif
