// The sensor-degradation stage between the renderer and the encoder: what a real depth camera does to the exact
// image scene.hip renders -- no-return pixels, range noise that grows with range, dropped pixels, erased boxes -- the
// reference's training augmentation (utils/data.py:11-108: additive Gaussian noise on the valid pixels, erased
// pixels and RandomErasing boxes, 0 the invalid value) as a reproducible function of (seed, stream, frame, pixel).
#include "philox.h"
#include "sensor_kernels.h"

namespace sdfn {

namespace {

// One pixel per lane, in place, no atomics and no state: one Philox call with the counter (pixel, frame, stream, 0)
// under the key seed.  Words 0 / 1 -> the Box-Muller uniforms in (0, 1], word 2 -> the dropout decision, an unsigned
// compare with the host's threshold.
__global__ __launch_bounds__(SENSOR_BLOCK) void sensor_degrade_kernel(SensorArgs A) {
    const int b = blockIdx.y;
    const int pix = (int)blockIdx.x * SENSOR_BLOCK + (int)threadIdx.x;
    if (pix >= A.H * A.W) return;
    float* p = A.img + (long long)b * A.H * A.W + pix;
    float v = *p;
    if (A.miss_invalid && v >= A.vmax) v = 0.f;  // no return
    const unsigned stream = A.stream_id ? (unsigned)A.stream_id[b] : (unsigned)b;
    unsigned w[4];
    philox4x32_10((unsigned)pix, A.frame, stream, 0u, A.key0, A.key1, w);
    if (v != 0.f) {  // an invalid pixel stays invalid (data.py:67)
        if (A.a != 0.f || A.b != 0.f) {
            const float u1 = (float)((w[0] >> 8) + 1u) * 0x1p-24f, u2 = (float)((w[1] >> 8) + 1u) * 0x1p-24f;
            const float z = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
            v = v + (A.a + A.b * v * v) * z;
        }
        v = fminf(fmaxf(v, 0.f), A.vmax);
    }
    if (w[2] < A.p_thresh) v = 0.f;
    if (A.boxes) {
        const int y = pix / A.W, x = pix - y * A.W;
        const int16_t* bx = A.boxes + ((long long)(A.frame % (unsigned)A.n_frames) * A.B + b) * A.max_boxes * 4;
        for (int i = 0; i < A.max_boxes; ++i) {
            const int y0 = bx[4 * i], x0 = bx[4 * i + 1], h = bx[4 * i + 2], wd = bx[4 * i + 3];
            if (y >= y0 && y < y0 + h && x >= x0 && x < x0 + wd) v = 0.f;  // h == 0: none
        }
    }
    *p = v;
}

}  // namespace

hipError_t launch_sensor_degrade(const SensorArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    const long long tiles = ((long long)a.H * a.W + SENSOR_BLOCK - 1) / SENSOR_BLOCK;
    hipLaunchKernelGGL(sensor_degrade_kernel, dim3((unsigned)tiles, (unsigned)a.B), dim3(SENSOR_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
