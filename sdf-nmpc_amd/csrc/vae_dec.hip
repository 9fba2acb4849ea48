// VAE decoder on gfx950: B latents -> B reconstructed range images.
//
// Reference: sdf_nmpc/network/vae.py:63-90 (Decoder), network/resnet.py:59-111 (ResBlockDeconv), eval mode:
// dropout is the identity and every BatchNorm is folded into its transposed convolution on the host
// (sdf-nmpc_amd/vae.py:decoder_layers), so the network is a chain of biased transposed convolutions.
//
// Kernels (activations channel-blocked [B][C / 16][H][W][16] as the encoder's, stored pre-split into three bf16
// planes hi / mid / lo, x = hi + mid + lo exactly; the 16 channels of a K-tile are 32 contiguous bytes of a pixel
// and a wave's rows -- consecutive pixels -- contiguous memory):
//   vae_dec_head_kernel    Linear(L, 512*8*15) + ELU, 4 images per workgroup, a thread per feature, the sum in
//                          a fixed order (bias, then l = 0 .. L-1)
//   vae_dec_gemm_kernel    every transposed convolution of the ResBlockDeconvs as an implicit GEMM over a tap
//                          list, on the bf16 matrix pipe with the encoder's fp32-exact split products:
//                            stride-1 3x3 ...... nine taps (the flipped kernel), one launch
//                            stride-2 3x3 ...... four output-parity phases of 1, 2, 2, 4 taps (blockIdx.y)
//                            stride-2 1x1 ...... one tap at the even-even phase; the same threads write the
//                                                folded BatchNorm shift into the other three phases
//                          256 x (32 WN) output tile per workgroup, K staged 16 at a time through registers
//                          into double-buffered LDS, bias / residual / ReLU fused into the epilogue
//   vae_dec_tail_kernel    ConvTranspose2d(32, 1, 5, s1, p2) on the vector ALU, a thread per logit
//   vae_dec_resize_kernel  bilinear resize (align_corners false) + sigmoid
#include <hip/hip_runtime.h>

#include <cstdint>

#include <math.h>

#include "vae_kernels.h"

namespace sdfn {

typedef float dec_floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 dec_bf16x8 __attribute__((ext_vector_type(8)));

// x = hi + mid + lo exactly, each a bf16 truncation of the remainder (vae_enc.hip:split3)
__device__ __forceinline__ void dec_split3(float x, unsigned& h, unsigned& m, unsigned& l) {
    h = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(h);
    m = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(m);
    l = __float_as_uint(r2) & 0xffff0000u;
}
__device__ __forceinline__ void dec_store4(unsigned short* pl, size_t ps, size_t o, float4 v) {
    unsigned h[4], m[4], l[4];
    dec_split3(v.x, h[0], m[0], l[0]);
    dec_split3(v.y, h[1], m[1], l[1]);
    dec_split3(v.z, h[2], m[2], l[2]);
    dec_split3(v.w, h[3], m[3], l[3]);
    *(uint2*)&pl[o] = make_uint2((h[0] >> 16) | h[1], (h[2] >> 16) | h[3]);
    *(uint2*)&pl[ps + o] = make_uint2((m[0] >> 16) | m[1], (m[2] >> 16) | m[3]);
    *(uint2*)&pl[2 * ps + o] = make_uint2((l[0] >> 16) | l[1], (l[2] >> 16) | l[3]);
}
__device__ __forceinline__ float dec_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float dec_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
// (hi + mid) + lo is the fp32 value exactly
__device__ __forceinline__ float4 dec_load4(const unsigned short* pl, size_t ps, size_t o) {
    const uint2 h = *(const uint2*)&pl[o], m = *(const uint2*)&pl[ps + o], l = *(const uint2*)&pl[2 * ps + o];
    return make_float4((dec_lo(h.x) + dec_lo(m.x)) + dec_lo(l.x), (dec_hi(h.x) + dec_hi(m.x)) + dec_hi(l.x),
                       (dec_lo(h.y) + dec_lo(m.y)) + dec_lo(l.y), (dec_hi(h.y) + dec_hi(m.y)) + dec_hi(l.y));
}

// ------------------------------------------------------------------------------------------------
// head: out[b][f] = ELU(bias[f] + sum_l wt[l][f] z[b][l]), f = (y, x, c), stored channel-blocked
constexpr int DH_IMG = 4;

__global__ __launch_bounds__(256) void vae_dec_head_kernel(VaeDecHeadArgs a) {
    __shared__ float zs[DH_IMG][VAE_DEC_LMAX];
    const int t = threadIdx.x, b0 = blockIdx.y * DH_IMG;
    for (int e = t; e < DH_IMG * a.L; e += 256) {
        const int q = e / a.L, l = e - q * a.L;
        zs[q][l] = b0 + q < a.B ? a.z[(size_t)(b0 + q) * a.L + l] : 0.f;
    }
    __syncthreads();
    const int f = blockIdx.x * 256 + t;
    if (f >= a.F) return;
    float acc[DH_IMG];
    const float bias = a.b[f];
#pragma unroll
    for (int q = 0; q < DH_IMG; ++q) acc[q] = bias;
    const float* w = a.wt + f;
#pragma unroll 4
    for (int l = 0; l < a.L; ++l) {
        const float wv = w[(size_t)l * a.F];
#pragma unroll
        for (int q = 0; q < DH_IMG; ++q) acc[q] = fmaf(wv, zs[q][l], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < DH_IMG; ++q) {
        if (b0 + q >= a.B) break;
        const float x = acc[q];
        const float y = !(x <= 0.f) ? x : expm1f(x);  // ELU(alpha = 1); a NaN stays a NaN
        unsigned h, m, l;
        dec_split3(y, h, m, l);
        // f = (pixel, c) -> channel-blocked [B][C / 16][pixels][16]
        const int pix = f / a.C, c = f - pix * a.C;
        const size_t o = (((size_t)(b0 + q) * (a.C >> 4) + (c >> 4)) * (a.F / a.C) + pix) * 16 + (c & 15);
        a.out[o] = (unsigned short)(h >> 16);
        a.out[a.ops + o] = (unsigned short)(m >> 16);
        a.out[2 * a.ops + o] = (unsigned short)(l >> 16);
    }
}

hipError_t launch_vae_dec_head(const VaeDecHeadArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.L < 1 || a.L > VAE_DEC_LMAX || a.F < 1 || a.C < 16 || a.C % 16 || a.F % a.C || !a.z || !a.wt || !a.b || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vae_dec_head_kernel, dim3((a.F + 255) / 256, (a.B + DH_IMG - 1) / DH_IMG), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// implicit GEMM over a tap list: for the phase ph = blockIdx.y and every cell (img, i, j) of the Hm x Wm grid,
//   out[img][os i + py][os j + px][n] = act(b[n] + sum_t sum_ci in[img][i + dy_t][j + dx_t][ci] W_t[ci][n] (+ resid))
// with a tap outside the input map contributing zeros.  m = (img, i, j) are the GEMM rows, k = (t, ci) in K-tiles
// of 16 channels of one tap.  Tile 256 x (32 WN): the four waves are stacked along m, each owning 64 rows (two
// 32x32 MFMA blocks) by all 32 WN channels.  A thread stages one row's 16 channels of the three planes (six
// 16-byte loads) and, the first 2 BN threads, half a row of the weight tile's planes; the next K-tile's loads are in flight in registers under the
// products of the current one, one barrier per K-tile.  LDS rows are 16 bf16 with the two halves of rows 8..15
// of every 16 swapped (vae_enc.hip:cv_off), so a fragment read's lane groups hit distinct 16-byte slots.
// The weight fragment is the MFMA's first operand: a lane ends with four consecutive channels of one pixel per
// register quad.  Six v_mfma_f32_32x32x16_bf16 per block and K-tile (al.bh, ah.bl, am.bm, am.bh, ah.bm, ah.bh),
// smallest first; the dropped products are <= 2^-24 relative.  Every row's sum runs over the same K order
// whatever tile it sits in, so an image does not depend on its batch neighbours.
constexpr int DG_BM = 256;
__device__ __forceinline__ int dg_off(int row, int half) { return row * 16 + 8 * (half ^ ((row >> 3) & 1)); }

template <int WN>
__global__ __launch_bounds__(256) void vae_dec_gemm_kernel(VaeDecGemmArgs a) {
    constexpr int BN = 32 * WN;
    __shared__ __align__(16) unsigned short As[2][3][DG_BM * 16];
    __shared__ __align__(16) unsigned short Bs[2][3][BN * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int ph = blockIdx.y;
    const int HWm = a.Hm * a.Wm, M = a.B * HWm, MT = (M + DG_BM - 1) / DG_BM;
    const int nt = blockIdx.x / MT, mt = blockIdx.x - nt * MT;
    const int CB = a.Cin >> 4, KT = a.ntaps[ph] * CB;

    // the row this thread stages
    const int m0 = mt * DG_BM + tid;
    const bool vm = m0 < M;
    const int q0 = vm ? m0 : 0, img0 = q0 / HWm, r0 = q0 - img0 * HWm, i0 = r0 / a.Wm, j0 = r0 - i0 * a.Wm;
    const unsigned short* wp = a.wpl + a.woff[ph] + (size_t)nt * BN * 16;
    const size_t wkt = (size_t)a.Cout * 16;  // elements per K-tile of a weight plane

    uint4 ra[6], rb0 = make_uint4(0, 0, 0, 0), rb1 = rb0, rb2 = rb0;
    auto fetch = [&](int kt) {
        const int t = kt / CB, cb = kt - t * CB;
        const int iy = i0 + a.dy[ph][t], ix = j0 + a.dx[ph][t];
        const bool ok = vm && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
        const unsigned short* p = a.in + ((((size_t)img0 * CB + cb) * a.Hi + (ok ? iy : 0)) * a.Wi + (ok ? ix : 0)) * 16;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            ra[2 * pl] = ok ? *(const uint4*)(p + pl * a.ips) : make_uint4(0, 0, 0, 0);
            ra[2 * pl + 1] = ok ? *(const uint4*)(p + pl * a.ips + 8) : make_uint4(0, 0, 0, 0);
        }
        if (BN == 128 || tid < BN * 2) {
            const unsigned short* q = wp + (size_t)kt * wkt + tid * 8;
            rb0 = *(const uint4*)q;
            rb1 = *(const uint4*)(q + a.wps);
            rb2 = *(const uint4*)(q + 2 * a.wps);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            *(uint4*)&As[buf][pl][dg_off(tid, 0)] = ra[2 * pl];
            *(uint4*)&As[buf][pl][dg_off(tid, 1)] = ra[2 * pl + 1];
        }
        if (BN == 128 || tid < BN * 2) {
            const int o = dg_off(tid >> 1, tid & 1);
            *(uint4*)&Bs[buf][0][o] = rb0;
            *(uint4*)&Bs[buf][1][o] = rb1;
            *(uint4*)&Bs[buf][2][o] = rb2;
        }
    };

    dec_floatx16 acc[2][WN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    fetch(0);
    stage(0);
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) fetch(kt + 1);
        dec_bf16x8 ah[2], am[2], al[2], bh[WN], bm[WN], bl[WN];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = dg_off(wave * 64 + 32 * i + lr, lh);
            ah[i] = *(const dec_bf16x8*)&As[buf][0][o];
            am[i] = *(const dec_bf16x8*)&As[buf][1][o];
            al[i] = *(const dec_bf16x8*)&As[buf][2][o];
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int o = dg_off(32 * j + lr, lh);
            bh[j] = *(const dec_bf16x8*)&Bs[buf][0][o];
            bm[j] = *(const dec_bf16x8*)&Bs[buf][1][o];
            bl[j] = *(const dec_bf16x8*)&Bs[buf][2][o];
        }
#define DG_MM(X, Y)                                                                                    \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < WN; ++j)        \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Y[j], X[i], acc[i][j], 0, 0, 0);
        DG_MM(al, bh)
        DG_MM(ah, bl)
        DG_MM(am, bm)
        DG_MM(am, bh)
        DG_MM(ah, bm)
        DG_MM(ah, bh)
#undef DG_MM
        if (kt + 1 < KT) stage(buf ^ 1);
        __syncthreads();
    }

    // epilogue: lane (lr, lh) holds cell 32 i + lr of the wave's rows and, in register quad g, channels
    // 32 j + 8 g + 4 lh .. + 3
    const int oy0 = a.py[ph], ox0 = a.px[ph];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = mt * DG_BM + wave * 64 + 32 * i + lr;
        if (m >= M) continue;
        const int img = m / HWm, r = m - img * HWm, ci = r / a.Wm, cj = r - ci * a.Wm;
        const int oy = a.os * ci + oy0, ox = a.os * cj + ox0;
        const size_t HWo = (size_t)a.Ho * a.Wo, pp = ((size_t)oy * a.Wo + ox) * 16;
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = nt * BN + 32 * j + 8 * g + 4 * lh;
                const float4 bias = *(const float4*)&a.b[n];
                // channel-blocked [B][Cout / 16][Ho][Wo][16]
                const size_t po = ((size_t)img * (a.Cout >> 4) + (n >> 4)) * HWo * 16 + pp + (n & 15);
                float4 v = make_float4(acc[i][j][4 * g] + bias.x, acc[i][j][4 * g + 1] + bias.y,
                                       acc[i][j][4 * g + 2] + bias.z, acc[i][j][4 * g + 3] + bias.w);
                if (a.resid) {
                    const float4 rv = dec_load4(a.resid, a.rps, po);
                    v = make_float4(v.x + rv.x, v.y + rv.y, v.z + rv.z, v.w + rv.w);
                }
                if (a.relu)  // torch.relu keeps a NaN (fmaxf would drop it)
                    v = make_float4(v.x < 0.f ? 0.f : v.x, v.y < 0.f ? 0.f : v.y, v.z < 0.f ? 0.f : v.z, v.w < 0.f ? 0.f : v.w);
                if (a.out) dec_store4(a.out, a.ops, po, v);
                if (a.out_f32)  // channel-quad planes [B][Cout / 4][Ho][Wo][4]: a wave's lanes write consecutive pixels
                    *(float4*)&a.out_f32[((((size_t)img * (a.Cout >> 2) + (n >> 2)) * a.Ho + oy) * a.Wo + ox) * 4] = v;
                if (a.fill3) {  // the stride-2 1x1 shortcut: the other three phases are the shift alone
                    const size_t row = (size_t)a.Wo * 16;
                    dec_store4(a.out, a.ops, po + 16, bias);
                    dec_store4(a.out, a.ops, po + row, bias);
                    dec_store4(a.out, a.ops, po + row + 16, bias);
                }
            }
    }
}

hipError_t launch_vae_dec_gemm(const VaeDecGemmArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!a.in || !a.wpl || !a.b || (!a.out && !a.out_f32) || a.Cin % 16 || a.Cout % 32 || a.nphase < 1 || a.nphase > 4 ||
        (a.os != 1 && a.os != 2) || ((uintptr_t)a.in & 15) || (a.ips & 7) || ((uintptr_t)a.wpl & 15) || (a.wps & 7) ||
        ((uintptr_t)a.b & 15))
        return hipErrorInvalidValue;
    for (int p = 0; p < a.nphase; ++p) {
        if (a.ntaps[p] < 1 || a.ntaps[p] > VAE_DEC_TAPS || (a.woff[p] & 7)) return hipErrorInvalidValue;
        // every cell's output pixel lies in the output map (the fill3 neighbours too)
        if (a.py[p] < 0 || a.px[p] < 0 || a.os * (a.Hm - 1) + a.py[p] + (a.fill3 ? 1 : 0) >= a.Ho ||
            a.os * (a.Wm - 1) + a.px[p] + (a.fill3 ? 1 : 0) >= a.Wo)
            return hipErrorInvalidValue;
    }
    if (a.fill3 && (!a.out || a.resid || a.relu)) return hipErrorInvalidValue;
    const long long M = (long long)a.B * a.Hm * a.Wm;
    const int bn = a.Cout % 128 == 0 ? 128 : a.Cout % 64 == 0 ? 64 : 32;
    const long long g = ((M + DG_BM - 1) / DG_BM) * (a.Cout / bn);
    if (M > 0x7fffffffLL || g > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)g, a.nphase);
    if (bn == 128)
        hipLaunchKernelGGL((vae_dec_gemm_kernel<4>), grid, dim3(256), 0, s, a);
    else if (bn == 64)
        hipLaunchKernelGGL((vae_dec_gemm_kernel<2>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((vae_dec_gemm_kernel<1>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// tail: ConvTranspose2d(C, 1, 5, s1, p2) = the 5x5 convolution with the flipped kernel,
//   logit[y][x] = b + sum_{ky, kx, ci} in[y + 2 - ky][x + 2 - kx][ci] w[ky][kx][ci],
// a thread per logit, the sum in the fixed order (ky, kx, ci) over the taps inside the map.  The input comes in
// channel-quad planes [B][C / 4][H][W][4] (the last GEMM's fp32 output), so the 64 lanes of a wave -- 64 consecutive
// columns of one row -- read 1 KB contiguous per load and the 25 taps' overlap is served by the caches
__global__ __launch_bounds__(256) void vae_dec_tail_kernel(VaeDecTailArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= a.W || y >= a.H) return;
    const int Q = a.C >> 2;
    const float4* in = (const float4*)a.in + (size_t)b * Q * a.H * a.W;
    float acc = a.b[0];
    for (int ky = 0; ky < 5; ++ky) {
        const int iy = y + 2 - ky;
        if ((unsigned)iy >= (unsigned)a.H) continue;
        for (int kx = 0; kx < 5; ++kx) {
            const int ix = x + 2 - kx;
            if ((unsigned)ix >= (unsigned)a.W) continue;
            const float4* p = in + (size_t)iy * a.W + ix;
            const float* w = a.w + (ky * 5 + kx) * a.C;
#pragma unroll 8
            for (int c = 0; c < Q; ++c) {
                const float4 v = p[(size_t)c * a.H * a.W];
                acc = fmaf(v.x, w[4 * c], acc);
                acc = fmaf(v.y, w[4 * c + 1], acc);
                acc = fmaf(v.z, w[4 * c + 2], acc);
                acc = fmaf(v.w, w[4 * c + 3], acc);
            }
        }
    }
    a.logits[((size_t)b * a.H + y) * a.W + x] = acc;
}

hipError_t launch_vae_dec_tail(const VaeDecTailArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!a.in || !a.w || !a.b || !a.logits || a.C % 4 || ((uintptr_t)a.in & 15) || a.B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vae_dec_tail_kernel, dim3((a.W + 63) / 64, (a.H + 3) / 4, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// Upsample(size, mode='bilinear', align_corners=False) in the formula of vae_pre_kernel, then the sigmoid
__global__ __launch_bounds__(256) void vae_dec_resize_kernel(VaeDecResizeArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.H * a.W) return;
    const int y = i / a.W, x = i - y * a.W;
    const float* in = a.logits + (size_t)b * a.Hi * a.Wi;
    float v;
    if (a.Hi == a.H && a.Wi == a.W) {
        v = in[i];
    } else {
        const float sh = (float)a.Hi / (float)a.H, sw = (float)a.Wi / (float)a.W;
        float fy = sh * ((float)y + 0.5f) - 0.5f, fx = sw * ((float)x + 0.5f) - 0.5f;
        fy = fy < 0.f ? 0.f : fy;
        fx = fx < 0.f ? 0.f : fx;
        int y0 = (int)fy, x0 = (int)fx;
        y0 = y0 > a.Hi - 1 ? a.Hi - 1 : y0;
        x0 = x0 > a.Wi - 1 ? a.Wi - 1 : x0;
        const int y1 = y0 + (y0 < a.Hi - 1), x1 = x0 + (x0 < a.Wi - 1);
        const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
        v = ly0 * (lx0 * in[y0 * a.Wi + x0] + lx1 * in[y0 * a.Wi + x1]) +
            ly1 * (lx0 * in[y1 * a.Wi + x0] + lx1 * in[y1 * a.Wi + x1]);
    }
    a.img[(size_t)b * a.H * a.W + i] = 1.f / (1.f + expf(-v));
}

hipError_t launch_vae_dec_resize(const VaeDecResizeArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!a.logits || !a.img || a.H < 1 || a.W < 1 || a.Hi < 1 || a.Wi < 1 || a.B > 65535 ||
        (long long)a.H * a.W > 0x7fffffffLL)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(vae_dec_resize_kernel, dim3((a.H * a.W + 255) / 256, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sdfn
