// Image morphology on batched [B][H][W] float32 images: the reference's Dilate / Erode / RemoveCloseOutliers
// (utils/preprocessing.py:100-259) as it writes them -- the padding by the element's origin with border value -2 /
// +2, Dilate's flipped mask over the unflipped padding, the excluded taps' bias of -2 / +2, ignore_zeros -- the same
// max / min over the same values, so the results are the reference's bit for bit.
#include "sensor_kernels.h"

namespace sdfn {

namespace {

// One output pixel per lane over a MORPH_TILE x MORPH_TILE tile.  The tile and a halo of the element's extent are
// staged in LDS with everything outside the image (and, with ignore_zeros, every zero) already replaced by the
// border value, so the tap loop is branch-free: acc = max / min(acc, tile[pixel + off[t]]) over the compact list of
// included taps, which every lane reads from the same LDS address (a broadcast).  The reference does not skip an
// excluded tap, it biases it by -2 / +2; such a tap wins only where every included tap reads the border value and
// the excluded pixel does not (an even-sized or asymmetric element at the image border, or among zeros under
// ignore_zeros).  The block keeps the extreme of its staged tile, and only a pixel whose result that extreme plus
// the bias could still beat scans the excluded taps as well.
__global__ __launch_bounds__(MORPH_BLOCK) void morph_kernel(MorphArgs A) {
    __shared__ float tile[MORPH_LDS_W * MORPH_LDS_W];
    __shared__ unsigned short tap[MORPH_K_MAX * MORPH_K_MAX];
    const int tid = threadIdx.x;
    const int lw = MORPH_TILE + A.k_w - 1, lh = MORPH_TILE + A.k_h - 1;
    const int x0 = (int)blockIdx.x * MORPH_TILE - A.ow, y0 = (int)blockIdx.y * MORPH_TILE - A.oh;
    const long long img = (long long)blockIdx.z * A.H * A.W;
    const float* src = A.in + img;
    __shared__ float wave_ext[MORPH_BLOCK / 64];
    const int n = A.taps.n, n_all = A.taps.n_all;
    const bool dilate = A.op == MORPH_DILATE;
    for (int i = tid; i < n_all; i += MORPH_BLOCK) tap[i] = A.taps.off[i];
    float ext = A.border;  // the largest (dilate) / smallest (erode) staged value
    for (int i = tid; i < lh * lw; i += MORPH_BLOCK) {
        const int r = i / lw, c = i - r * lw;
        const int y = y0 + r, x = x0 + c;
        float v = A.border;
        if (y >= 0 && y < A.H && x >= 0 && x < A.W) {
            v = src[y * A.W + x];
            if (A.ignore_zeros && v == 0.f) v = A.border;
        }
        tile[i] = v;
        ext = dilate ? fmaxf(ext, v) : fminf(ext, v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float o = __shfl_xor(ext, m, 64);
        ext = dilate ? fmaxf(ext, o) : fminf(ext, o);
    }
    if ((tid & 63) == 0) wave_ext[tid >> 6] = ext;
    __syncthreads();
    const int lx = tid & (MORPH_TILE - 1), ly = tid / MORPH_TILE;
    const int x = (int)blockIdx.x * MORPH_TILE + lx, y = (int)blockIdx.y * MORPH_TILE + ly;
    if (x >= A.W || y >= A.H) return;
    const float* t0 = tile + ly * lw + lx;
    float acc = t0[tap[0]];
    if (dilate) {
        for (int t = 1; t < n; ++t) acc = fmaxf(acc, t0[tap[t]]);
        const float best = fmaxf(fmaxf(wave_ext[0], wave_ext[1]), fmaxf(wave_ext[2], wave_ext[3])) + A.border;
        if (acc < best)
            for (int t = n; t < n_all; ++t) acc = fmaxf(acc, t0[tap[t]] + A.border);
    } else {
        for (int t = 1; t < n; ++t) acc = fminf(acc, t0[tap[t]]);
        const float best = fminf(fminf(wave_ext[0], wave_ext[1]), fminf(wave_ext[2], wave_ext[3])) + A.border;
        if (acc > best)
            for (int t = n; t < n_all; ++t) acc = fminf(acc, t0[tap[t]] + A.border);
    }
    if (A.ignore_zeros && acc == A.border) acc = 0.f;
    A.out[img + y * A.W + x] = acc;
}

// RemoveCloseOutliers(kernel_size = 3, min_range) in one pass: t = in < min_range ? 0 : in on the tile and a halo of
// two pixels (outside the image: the erosion's border +2); e = the 3 x 3 erosion of t on the tile and a halo of one
// (outside the image: the dilation's border -2, not an erosion of padding); d = the 3 x 3 dilation of e;
// out = d > 0 ? t : d.  No intermediate image leaves the block.
constexpr int OR_T = MORPH_TILE + 4, OR_E = MORPH_TILE + 2;

__global__ __launch_bounds__(MORPH_BLOCK) void outlier_rm_kernel(OutlierArgs A) {
    __shared__ float t[OR_T * OR_T];
    __shared__ float e[OR_E * OR_E];
    const int tid = threadIdx.x;
    const int bx = (int)blockIdx.x * MORPH_TILE, by = (int)blockIdx.y * MORPH_TILE;
    const long long img = (long long)blockIdx.z * A.H * A.W;
    const float* src = A.in + img;
    for (int i = tid; i < OR_T * OR_T; i += MORPH_BLOCK) {
        const int r = i / OR_T, c = i - r * OR_T;
        const int y = by - 2 + r, x = bx - 2 + c;
        float v = 2.f;
        if (y >= 0 && y < A.H && x >= 0 && x < A.W) {
            v = src[y * A.W + x];
            v = v < A.min_range ? 0.f : v;
        }
        t[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < OR_E * OR_E; i += MORPH_BLOCK) {
        const int r = i / OR_E, c = i - r * OR_E;
        const int y = by - 1 + r, x = bx - 1 + c;
        float m = -2.f;
        if (y >= 0 && y < A.H && x >= 0 && x < A.W) {
            const float* p = t + r * OR_T + c;
            m = p[0];
#pragma unroll
            for (int dr = 0; dr < 3; ++dr)
#pragma unroll
                for (int dc = 0; dc < 3; ++dc) m = fminf(m, p[dr * OR_T + dc]);
        }
        e[i] = m;
    }
    __syncthreads();
    const int lx = tid & (MORPH_TILE - 1), ly = tid / MORPH_TILE;
    const int x = bx + lx, y = by + ly;
    if (x >= A.W || y >= A.H) return;
    const float* p = e + ly * OR_E + lx;
    float d = p[0];
#pragma unroll
    for (int dr = 0; dr < 3; ++dr)
#pragma unroll
        for (int dc = 0; dc < 3; ++dc) d = fmaxf(d, p[dr * OR_E + dc]);
    A.out[img + y * A.W + x] = d > 0.f ? t[(ly + 2) * OR_T + lx + 2] : d;
}

__global__ __launch_bounds__(256) void morph_threshold_kernel(const float* in, float* out, long long n, float min_range) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = in[i];
    out[i] = v < min_range ? 0.f : v;
}

__global__ __launch_bounds__(256) void morph_restore_kernel(float* img, const float* t, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float d = img[i];
    if (d > 0.f) img[i] = t[i];
}

inline dim3 tile_grid(int B, int H, int W) {
    return dim3((unsigned)((W + MORPH_TILE - 1) / MORPH_TILE), (unsigned)((H + MORPH_TILE - 1) / MORPH_TILE), (unsigned)B);
}

}  // namespace

hipError_t launch_morph(const MorphArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(morph_kernel, tile_grid(a.B, a.H, a.W), dim3(MORPH_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_outlier_rm(const OutlierArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(outlier_rm_kernel, tile_grid(a.B, a.H, a.W), dim3(MORPH_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_morph_threshold(const float* in, float* out, long long n, float min_range, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(morph_threshold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n, min_range);
    return hipGetLastError();
}

hipError_t launch_morph_restore(float* img, const float* t, long long n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(morph_restore_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, img, t, n);
    return hipGetLastError();
}

}  // namespace sdfn
