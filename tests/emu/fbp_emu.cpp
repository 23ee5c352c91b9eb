// Host build of csrc/fbp_core.h: the loops of the gfx950 kernels (csrc/fbp.hip) over image lines and over
// a volume, one element at a time.  Compiled by tests/test_fbp.py with g++; no HIP, no GPU.
#include <vector>

#include "../../diffdrr_amd/csrc/fbp_core.h"

extern "C" {

void fbp_emu_filter(const float *images, int B, int H, int W, int axis, const float *taps, float scale, float u0,
                    float du, float v0, float dv, float sdd, int cosine_weight, float *out) {
    const int L = axis == 0 ? W : H, across = axis == 0 ? H : W;
    std::vector<float> line(L > 0 ? L : 1);
    for (long id = 0; id < (long)B * across; ++id) {
        const long b = id / across;
        const int at = (int)(id - b * across);
        const long first = axis == 0 ? (b * H + at) * W : b * H * W + at, step = axis == 0 ? 1 : W;
        for (int k = 0; k < L; ++k)
            line[k] = fbp::weighted_pixel(images[first + k * step], axis == 0 ? at : k, axis == 0 ? k : at, u0, du,
                                          v0, dv, sdd, cosine_weight);
        for (int n = 0; n < L; ++n) out[first + n * step] = fbp::convolve(line.data(), taps, L, n, scale);
    }
}

void fbp_emu_backproject(const float *images, int B, int H, int W, const float *views, int distance_weight,
                         float *volume, int Dx, int Dy, int Dz, int accumulate) {
    if (H == 0 || W == 0) B = 0;
    for (int i = 0; i < Dx; ++i)
        for (int j = 0; j < Dy; ++j)
            for (int k = 0; k < Dz; ++k) {
                float acc = 0.f;
                for (int b = 0; b < B; ++b) {
                    const float *view = views + (long)b * 16;
                    acc = fbp::accumulate_view(acc, images + (long)b * H * W, H, W, view, fbp::row_of(view, i, j), k,
                                               distance_weight);
                }
                float &dst = volume[((long)i * Dy + j) * Dz + k];
                dst = accumulate ? dst + acc : acc;
            }
}

}  // extern "C"
