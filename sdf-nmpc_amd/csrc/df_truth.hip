// Ground truth from range images: what the image itself says about a point, next to what the network
// conditioned on it predicts.  Restates the reference's two NVIDIA-Warp kernels as written, quirks included:
//
//   colcheck_kernel   utils/collision_checker.py:23-90   ColChecker._kernel_colcheck
//   minpool5_kernel   utils/df_computer.py:154-162       the zero-skipping 5x5 min-pool of get_udf
//   udf_kernel        utils/df_computer.py:102-149,177-180  _kernel_pixel_wise_udf + the min / gradient
//   sdf_grid_kernel   utils/df_computer.py:200-221       get_sdf, fused: no n x G buffer exists
//   img_sdf_rows      gen_model.py:46-61 on df_computer.py:152-221: sdf_grid_kernel / udf_kernel in their rows mode, at
//                     the node positions of a batch, written as the SDF row of h / J_h -- the controller flying
//                     on the network's own training labels (DfComputer.get_df), no network
//
// fp32 throughout (Warp float32).  Reductions are (value, index) minima with ties to the lowest index,
// in-wave by shuffles and across waves through LDS: no atomics, so results do not depend on scheduling.
#include "cam_point.h"
#include "df_kernels.h"

#include <climits>

namespace sdfn {

namespace {

struct ImgCfg {
    float dmax, hfov, vfov, tan_h, tan_v;
    int is_depth, is_spherical, H, W;
};

__device__ __forceinline__ ImgCfg img_cfg(float dmax, float hfov, float vfov, int is_depth, int is_spherical, int H,
                                          int W) {
    // tan(hfov), tan(vfov): launch constants of collision_checker.py:83-84
    return ImgCfg{dmax, hfov, vfov, tanf(hfov), tanf(vfov), is_depth, is_spherical, H, W};
}

__device__ __forceinline__ ImgCfg img_cfg(const DfImg& im) {
    return img_cfg(im.dmax, im.hfov, im.vfov, im.is_depth, im.is_spherical, im.H, im.W);
}

__device__ __forceinline__ const float* img_of(const DfImg& im, long long j) {
    const long long i = im.p_to_i ? (long long)im.p_to_i[j] : j / im.per_img;  // entries are the caller's to keep in range
    return im.img + (size_t)i * im.H * im.W;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }  // wp.clamp

// clamp(int(f), 0, n - 1) with int() truncating toward zero (collision_checker.py:80-84), written so that a
// value outside int's range (tan near pi/2) or a NaN still lands on a pixel of the image
__device__ __forceinline__ int pix_of(float f, int n) { return !(f > 0.f) ? 0 : f >= (float)n ? n - 1 : (int)f; }

// collision_checker.py:47-90 for one point against its image
__device__ __forceinline__ int col_test(const float* __restrict__ img, const ImgCfg& c, int outside, float safe_ball,
                                        float x, float y, float z) {
    const float len = sqrtf(x * x + y * y + z * z);
    if (!(len > safe_ball)) return 0;              // :47 inside the safe ball: free
    const float val = c.is_depth ? x : len;        // :49-52
    if (val >= c.dmax) return 1;                   // :54 past dmax is unsafe
    float az = atan2f(y, x);                       // :58
    float el = c.is_spherical ? atan2f(z, sqrtf(x * x + y * y)) : atan2f(z, x);  // :59-62
    if (outside == 2) {                            // :64-66 extrapolate
        az = clampf(az, -c.hfov, c.hfov);
        el = clampf(el, -c.vfov, c.vfov);
    } else if (fabsf(az) >= c.hfov || fabsf(el) >= c.vfov) {  // :68-72
        return outside == 1;
    }
    const float w = (float)c.W, h = (float)c.H;
    float fu, fv;
    if (c.is_spherical) {                          // :79-81
        fu = w / 2.f * (1.f - az / c.hfov);
        fv = h / 2.f * (1.f - el / c.vfov);
    } else {                                       // :82-84
        fu = w / 2.f * (1.f - tanf(az) / c.tan_h);
        fv = h / 2.f * (1.f - tanf(el) / c.tan_v);
    }
    const int u = pix_of(fu, c.W), v = pix_of(fv, c.H);
    return val >= img[(size_t)v * c.W + u] * c.dmax;  // :89 (a zero pixel always collides)
}

// minimum of (d, i) in lexicographic order over the workgroup; pos rides along.  Result valid in thread 0.
__device__ __forceinline__ void lexmin(float& d, int& i, int& pos, float d2, int i2, int pos2) {
    if (d2 < d || (d2 == d && i2 < i)) {
        d = d2;
        i = i2;
        pos = pos2;
    }
}

__device__ __forceinline__ void block_lexmin(float& d, int& i, int& pos, float* sd, int* si, int* sp) {
    for (int o = 32; o > 0; o >>= 1) lexmin(d, i, pos, __shfl_xor(d, o), __shfl_xor(i, o), __shfl_xor(pos, o));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sd[wave] = d;
        si[wave] = i;
        sp[wave] = pos;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < DF_BLOCK / 64; ++k) lexmin(d, i, pos, sd[k], si[k], sp[k]);
}

__global__ __launch_bounds__(DF_BLOCK) void colcheck_kernel(ColcheckArgs a) {
    const long long j = (long long)blockIdx.x * DF_BLOCK + threadIdx.x;
    if (j >= a.im.n) return;
    const ImgCfg c = img_cfg(a.im);
    const float* p = a.im.points + (size_t)j * 3;
    a.out[j] = (unsigned char)col_test(img_of(a.im, j), c, a.outside, a.safe_ball, p[0], p[1], p[2]);
}

// df_computer.py:154-162: zeros (invalid pixels) are replaced by dmax -- the unnormalised dmax, as written --
// before the minimum, unless the whole 5x5 block is zero, which stays 0
__global__ __launch_bounds__(DF_BLOCK) void minpool5_kernel(MinpoolArgs a) {
    const int h = a.H / 5, w = a.W / 5;
    const long long k = (long long)blockIdx.x * DF_BLOCK + threadIdx.x;
    if (k >= (long long)a.n_img * h * w) return;
    const int i = (int)(k % w), j = (int)(k / w % h);
    const long long b = k / ((long long)w * h);
    const float* src = a.img + ((size_t)b * a.H + (size_t)j * 5) * a.W + (size_t)i * 5;
    float m = INFINITY;
    int nz = 0;
    for (int r = 0; r < 5; ++r)
        for (int q = 0; q < 5; ++q) {
            const float v = src[(size_t)r * a.W + q];
            nz += v != 0.f;
            m = fminf(m, v == 0.f ? a.dmax : v);
        }
    a.out[k] = nz ? m : 0.f;
}

// distance of point p to pooled pixel k and the direction the gradient is taken from (df_computer.py:118-149).
// col / row hold the launch's pixel directions: col[2i], col[2i+1] and row[2j], row[2j+1] (udf_kernel).
__device__ __forceinline__ float udf_pix(const float* __restrict__ img, const ImgCfg& c, const float* col,
                                         const float* row, int k, float px, float py, float pz, float d_bg,
                                         float& dx, float& dy, float& dz) {
    const int i = k % c.W, j = k / c.W;
    float x, y, z;
    if (c.is_spherical) {  // :121-124 (sic: the reference's is_spherical branch is the pinhole direction)
        x = 1.f;
        y = col[2 * i];
        z = row[2 * j];
    } else {               // :127-131
        x = row[2 * j] * col[2 * i];
        y = row[2 * j] * col[2 * i + 1];
        z = row[2 * j + 1];
    }
    const float s = img[k];
    dx = x * s * c.dmax - px;  // :125,132,134
    dy = y * s * c.dmax - py;
    dz = z * s * c.dmax - pz;
    // the reference's `x == 0` branch (:136-137) is dead: x is 1 or a product of fp32 cosines of angles
    // that are never exactly pi/2
    const float d_p = sqrtf(dx * dx + dy * dy + dz * dz);
    if (d_p > d_bg) {  // :145-147 closer to the virtual wall at dmax; the direction is the reference's
        dx = c.dmax;
        dy = py;
        dz = pz;
        return d_bg;
    }
    return d_p;
}

// gen_model.py:46-61 with the image's own field in the place of the network: h[r][2] = flag df + (1 - flag) max_df and
// J_h[r][j][2] = flag (W_R_Co g)_j, df and the camera-frame gradient g widened from fp32.  fp64, no contraction: a host
// restatement of these statements gives the same bits.
__device__ __forceinline__ void img_sdf_epilogue(double flag, float df, float g0, float g1, float g2, const double* R,
                                                 double max_df, double* h2, double* J) {
#pragma clang fp contract(off)
    const double d = (double)df, a0 = (double)g0, a1 = (double)g1, a2 = (double)g2;
    *h2 = flag * d + (1.0 - flag) * max_df;
#pragma unroll
    for (int j = 0; j < 3; ++j) J[j * 3] = flag * ((R[3 * j] * a0 + R[3 * j + 1] * a1) + R[3 * j + 2] * a2);
#pragma unroll
    for (int j = 3; j < 10; ++j) J[j * 3] = 0.0;
}

// The image field as the SDF row ("img_sdf_rows"; launch_img_sdf_rows) is udf_kernel / sdf_grid_kernel themselves with
// r.x != nullptr: point pt is then node row pt = b (N+1) + k.  rows_prologue: thread 0 forms the row's camera-frame
// point (cam_point, the network kernels' statements) and stores it where the scan reads its point from (a.im.points:
// the caller's pts or a workspace); where the flag is 0 the row is written at once and the scan skipped (false is
// returned, uniformly); else a barrier makes the point visible.  After the scan thread 0 writes img_sdf_epilogue
// instead of (df, grad).  One kernel per field, so that the scan of a row is the very machine code that labels a point:
// the same bits by construction, whatever the compiler fuses.
__device__ __forceinline__ bool rows_prologue(const DfRowsArgs& r, long long pt, float max_df, double& flag) {
    const double* pr = r.p + (size_t)pt * r.np;
    flag = pr[0];
    if (threadIdx.x == 0) {  // the point of every row, whatever its flag
        const float4 P = cam_point(r.x + (size_t)pt * 10, pr);
        float* w = r.pts + (size_t)pt * 3;  // == a.im.points + 3 pt
        w[0] = P.x;
        w[1] = P.y;
        w[2] = P.z;
    }
    if (flag == 0.0) {  // uniform over the workgroup.  The field is always finite (clamped), so the epilogue would give
        // 0 df + 1 max_df = max_df, the same bits, and flag (..) = a zero (of either sign)
        if (threadIdx.x == 0) {
            r.h[pt * 3 + 2] = (double)max_df;
#pragma unroll
            for (int j = 0; j < 10; ++j) r.Jh[pt * 30 + j * 3 + 2] = 0.0;
        }
        return false;
    }
    __syncthreads();  // thread 0's point is visible to the workgroup
    return true;
}

// the image of row pt: instance b = pt / N1 reads image b, or img_of[b] (entries are the caller's to keep in range)
__device__ __forceinline__ const float* rows_img(const DfImg& im, const DfRowsArgs& r, long long pt) {
    const long long b = pt / r.N1;
    return im.img + (size_t)(r.img_of ? (long long)r.img_of[b] : b) * im.H * im.W;
}

__global__ __launch_bounds__(DF_BLOCK) void udf_kernel(UdfArgs a, DfRowsArgs r) {
    extern __shared__ float tab[];  // col [2 w] | row [2 h]
    __shared__ float sd[DF_BLOCK / 64];
    __shared__ int si[DF_BLOCK / 64], sp[DF_BLOCK / 64];
    const ImgCfg c = img_cfg(a.im);
    const int w = c.W, h = c.H;
    float* col = tab;
    float* row = tab + 2 * w;
    // the pixel directions depend on the launch only: once per workgroup, separably (w + h entries)
    for (int t = threadIdx.x; t < w + h; t += DF_BLOCK) {
        const bool is_col = t < w;
        const float f = 1.f - 2.f * (float)(is_col ? t : t - w) / (float)(is_col ? w : h);
        float* dst = is_col ? col + 2 * t : row + 2 * (t - w);
        if (c.is_spherical) {
            dst[0] = (is_col ? c.tan_h : c.tan_v) * f;  // :123-124
            dst[1] = 0.f;
        } else {
            const float ang = (is_col ? c.hfov : c.vfov) * f;  // :127-128
            dst[0] = cosf(ang);
            dst[1] = sinf(ang);
        }
    }
    __syncthreads();
    const long long pt = blockIdx.x;
    double flag = 1.0;
    if (r.x && !rows_prologue(r, pt, a.max_df, flag)) return;
    const float* p = a.im.points + (size_t)pt * 3;
    const float px = p[0], py = p[1], pz = p[2];
    const float* img = r.x ? rows_img(a.im, r, pt) : img_of(a.im, pt);
    const float d_bg = c.dmax - (c.is_depth ? px : sqrtf(px * px + py * py + pz * pz));  // :140-143
    float best = INFINITY;
    int bi = INT_MAX, bp = 0;
    for (int k = threadIdx.x; k < w * h; k += DF_BLOCK) {
        float dx, dy, dz;
        const float d = udf_pix(img, c, col, row, k, px, py, pz, d_bg, dx, dy, dz);
        lexmin(best, bi, bp, d, k, k);
    }
    block_lexmin(best, bi, bp, sd, si, sp);
    if (threadIdx.x == 0) {
        if (bi == INT_MAX) bi = 0;  // every distance NaN: torch.min's index is unspecified; take pixel 0
        float dx, dy, dz;
        const float d = udf_pix(img, c, col, row, bi, px, py, pz, d_bg, dx, dy, dz);
        const float udf = clampf(d, 0.f, a.max_df);  // :178
        const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
        const bool sat = udf == a.max_df;            // :180
        if (r.x) {
            img_sdf_epilogue(flag, udf, sat ? 0.f : -(dx / nrm), sat ? 0.f : -(dy / nrm), sat ? 0.f : -(dz / nrm),
                             r.p + (size_t)pt * r.np + 4, (double)a.max_df, r.h + pt * 3 + 2, r.Jh + pt * 30 + 2);
            return;
        }
        a.udf[pt] = udf;
        a.grad[pt * 3 + 0] = sat ? 0.f : -(dx / nrm);
        a.grad[pt * 3 + 1] = sat ? 0.f : -(dy / nrm);
        a.grad[pt * 3 + 2] = sat ? 0.f : -(dz / nrm);
        if (a.pix_idx) a.pix_idx[pt] = bi;
    }
}

// df_computer.py:200-221 for the point (px, py, pz) by the whole workgroup.  A voxel counts when its collision label
// differs from the point's (_get_mindist_occgrid, :193-197); the result is the counting voxel of least dist, ties to
// the lowest voxel index.  With orig_idx the grid is sorted by dist: the scan stops after the first chunk that
// holds a counting voxel and the chunks that may still hold one at the same dist.  Every argument is uniform over
// the workgroup (the loop holds barriers); results valid in thread 0, vox = -1 where no voxel counts.
__device__ __forceinline__ void sdf_grid_point(const float* __restrict__ img, const ImgCfg& c, float px, float py,
                                               float pz, float min_df, float max_df, const float* grid,
                                               const float* dist, const int* orig_idx, int G, float* sd, int* si,
                                               int* sp, float& sdf, float& gx, float& gy, float& gz, int& vox) {
    const int occ = col_test(img, c, 2, 0.f, px, py, pz);  // :201, ColChecker(.., 0, .., 'extrapolate') (:22)
    const bool sorted = orig_idx != nullptr;
    float best = INFINITY;
    int bi = INT_MAX, bp = 0;
    bool stopping = false;
    float stop_d = 0.f;
    for (int base = 0; base < G; base += DF_BLOCK) {
        if (stopping && !(dist[base] <= stop_d)) break;  // uniform: every later voxel is farther
        const int g = base + (int)threadIdx.x;
        if (g < G) {
            const float* v = grid + (size_t)g * 3;
            if (col_test(img, c, 2, 0.f, px + v[0], py + v[1], pz + v[2]) != occ)  // :188,213
                lexmin(best, bi, bp, dist[g], sorted ? orig_idx[g] : g, g);
        }
        if (sorted && !stopping && __syncthreads_or(bi != INT_MAX)) {
            stopping = true;
            stop_d = dist[min(base + DF_BLOCK, G) - 1];  // no found voxel is farther than this one
        }
    }
    block_lexmin(best, bi, bp, sd, si, sp);
    if (threadIdx.x == 0) {
        const bool found = bi != INT_MAX;
        const float sign = occ ? -1.f : 1.f;                                     // :202
        sdf = clampf(sign * (found ? best : max_df), min_df, max_df);            // :195,217
        const bool sat = !found || sdf == min_df || sdf == max_df;               // :219
        gx = 0.f, gy = 0.f, gz = 0.f;
        if (!sat) {
            const float* v = grid + (size_t)bp * 3;
            const float nrm = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);   // :218
            gx = -sign * (v[0] / nrm);
            gy = -sign * (v[1] / nrm);
            gz = -sign * (v[2] / nrm);
        }
        vox = found ? bi : -1;
    }
}

__global__ __launch_bounds__(DF_BLOCK) void sdf_grid_kernel(SdfGridArgs a, DfRowsArgs r) {
    __shared__ float sd[DF_BLOCK / 64];
    __shared__ int si[DF_BLOCK / 64], sp[DF_BLOCK / 64];
    const ImgCfg c = img_cfg(a.im);
    const long long pt = blockIdx.x;
    double flag = 1.0;
    if (r.x && !rows_prologue(r, pt, a.max_df, flag)) return;
    const float* p = a.im.points + (size_t)pt * 3;
    float sdf = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    int vox = -1;
    sdf_grid_point(r.x ? rows_img(a.im, r, pt) : img_of(a.im, pt), c, p[0], p[1], p[2], a.min_df, a.max_df, a.grid, a.dist,
                   a.orig_idx, a.G, sd, si, sp, sdf, gx, gy, gz, vox);
    if (threadIdx.x == 0) {
        if (r.x) {
            img_sdf_epilogue(flag, sdf, gx, gy, gz, r.p + (size_t)pt * r.np + 4, (double)a.max_df, r.h + pt * 3 + 2,
                             r.Jh + pt * 30 + 2);
            return;
        }
        a.sdf[pt] = sdf;
        a.grad[pt * 3 + 0] = gx;
        a.grad[pt * 3 + 1] = gy;
        a.grad[pt * 3 + 2] = gz;
        if (a.vox_idx) a.vox_idx[pt] = vox;
    }
}

}  // namespace

hipError_t launch_colcheck(const ColcheckArgs& a, hipStream_t s) {
    const long long blocks = (a.im.n + DF_BLOCK - 1) / DF_BLOCK;
    hipLaunchKernelGGL(colcheck_kernel, dim3((unsigned)blocks), dim3(DF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_minpool5(const MinpoolArgs& a, hipStream_t s) {
    const long long n = (long long)a.n_img * (a.H / 5) * (a.W / 5);
    hipLaunchKernelGGL(minpool5_kernel, dim3((unsigned)((n + DF_BLOCK - 1) / DF_BLOCK)), dim3(DF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_udf(const UdfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(udf_kernel, dim3((unsigned)a.im.n), dim3(DF_BLOCK), udf_lds_bytes(a.im.H, a.im.W), s, a,
                       DfRowsArgs{});
    return hipGetLastError();
}

hipError_t launch_sdf_grid(const SdfGridArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(sdf_grid_kernel, dim3((unsigned)a.im.n), dim3(DF_BLOCK), 0, s, a, DfRowsArgs{});
    return hipGetLastError();
}

// the labelling kernels in their rows mode: the points buffer a.pts is the rows' own (required)
hipError_t launch_img_sdf_rows(const ImgSdfArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const DfRowsArgs r{a.x, a.p, a.h, a.Jh, a.pts, a.img_of, a.N1, a.np};
    if (a.is_signed) {
        SdfGridArgs g{};
        g.im = DfImg{a.images, 0, a.H, a.W, a.dmax, a.hfov, a.vfov, a.is_depth, a.is_spherical, a.pts, nullptr, a.rows, a.N1};
        g.min_df = a.min_df; g.max_df = a.max_df;
        g.grid = a.grid; g.dist = a.dist; g.orig_idx = a.orig_idx; g.G = a.G;
        hipLaunchKernelGGL(sdf_grid_kernel, dim3((unsigned)a.rows), dim3(DF_BLOCK), 0, s, g, r);
    } else {  // on the pooled images
        const int h = a.H / 5, w = a.W / 5;
        UdfArgs u{};
        u.im = DfImg{a.pooled, 0, h, w, a.dmax, a.hfov, a.vfov, a.is_depth, a.is_spherical, a.pts, nullptr, a.rows, a.N1};
        u.max_df = a.max_df;
        hipLaunchKernelGGL(udf_kernel, dim3((unsigned)a.rows), dim3(DF_BLOCK), udf_lds_bytes(h, w), s, u, r);
    }
    return hipGetLastError();
}

}  // namespace sdfn
