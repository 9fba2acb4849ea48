// Device code shared by the two row evaluators (sdf_row.hip: the deployed network with compile-time shapes;
// sdf_row_wide.hip: every other network): the opaque copies that keep the server's request loop free of
// spills, the lane sums, the position embedding and its contraction, and the resident server's mailbox
// protocol (SdfMbox, sdf_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sdf_kernels.h"
#include "sincos.h"

namespace sdfn {

// The weight pointer of a layer is laundered at the layer: in the resident server's request loop the
// compiler would otherwise issue every layer's weight loads up front (or hoist them out of the loop)
// and spill them to scratch.
template <typename T>
__device__ __forceinline__ const T* launder(const T* p) {
    asm volatile("" : "+s"(p));
    return p;
}

// threadIdx.x behind an opaque copy: in the server's request loop the compiler would otherwise hoist
// every lane-dependent index and address of the evaluation out of the loop and spill them
__device__ __forceinline__ int tix() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over aligned groups of QR lanes (QR = 4, 8 or 16, inside one DPP row), every lane of a group
// receiving the group's sum: quad butterflies, then the half-row and row mirrors
template <int QR>
__device__ __forceinline__ float group_sum(float v) {
    static_assert(QR == 4 || QR == 8 || QR == 16, "group of 4, 8 or 16 lanes");
    auto dpp = [](float x, auto ctrl) {
        constexpr int C = decltype(ctrl)::value;
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), C, 0xf, 0xf, false));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});  // quad_perm [1, 0, 3, 2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});  // quad_perm [2, 3, 0, 1]
    if constexpr (QR >= 8) v += dpp(v, std::integral_constant<int, 0x141>{});  // row_half_mirror
    if constexpr (QR >= 16) v += dpp(v, std::integral_constant<int, 0x140>{});  // row_mirror
    return v;
}

// feature m of the embedding e = [x, sin(xb), sin(xb + pi/2)] of position p, and d e / d xb (1 for the
// position itself): nb projected frequencies, tab[m] = (dir * 2^f, 0) their rows; features from 3 + 2 nb
// on are padding (0, 0).  The arithmetic is sdf_mlp.hip's / sdf_wide.hip's.
__device__ __forceinline__ void embed_feature(const float4 p, const int m, const int nb, const float4* tab, float& e,
                                              float& g) {
    e = 0.0f;
    g = 0.0f;
    if (m < 3) {
        e = m == 0 ? p.x : (m == 1 ? p.y : p.z);
        g = 1.0f;
    } else if (m < 3 + 2 * nb) {
        const float4 t = tab[m];
        float xb = p.x * t.x + p.y * t.y + p.z * t.z;
        if (m >= 3 + nb) xb = xb + 1.57079637050628662109375f;
        sdfn_sincosf(xb, &e, &g);
    }
}

// d df / d pos through the embedding, by one wave: sum over the n features of (ga[m] + gb[m]) gm[m] times
// d xb_m / d pos (tab[m]; the identity for the position's own three features); every lane gets the sums
__device__ __forceinline__ void dpos_sum(const float* ga, const float* gb, const float* gm, const float4* tab,
                                         const int n, const int lane, float& s0, float& s1, float& s2) {
    s0 = s1 = s2 = 0.0f;
    for (int m = lane; m < n; m += 64) {
        const float u = (ga[m] + gb[m]) * gm[m];
        if (m < 3) {
            s0 += m == 0 ? u : 0.0f;
            s1 += m == 1 ? u : 0.0f;
            s2 += m == 2 ? u : 0.0f;
        } else {
            const float4 t = tab[m];
            s0 = fmaf(u, t.x, s0);
            s1 = fmaf(u, t.y, s1);
            s2 = fmaf(u, t.z, s2);
        }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
}

// system-scope (host-coherent) accesses of the mailbox: vector loads / stores that bypass the GPU caches
__device__ __forceinline__ unsigned long long mb_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned int mb_load_u32(const unsigned int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void mb_store(long long* p, long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the per-call fields of a request the server staged: [rows][4] | [rows][LH] in s_in, the results in the
// same layout in s_out
__device__ __forceinline__ RowCall staged_call(const float* s_in, float* s_out, const int rows, const int grad) {
    return RowCall{(const float4*)s_in, s_in + rows * 4, (float4*)s_out, grad ? s_out + rows * 4 : nullptr, rows};
}

// The resident server (SdfMbox, sdf_kernels.h), run by one workgroup of WT threads: thread 0 polls seq_in;
// the request (at most max_rows rows of 4 + LH floats) is staged into LDS (s_in) with one PCIe read per
// word; eval(rows, grad) evaluates the rows from s_in into s_out (staged_call); the results go to the
// mailbox with write-through stores, and seq_out publishes them.  Every exit path (stop, idle, life) is
// taken by the whole workgroup together (the decision goes through LDS behind a barrier), between
// requests, and ends with the launch's epoch stored to `gone`, so a caller that posted a request the
// leaving server did not see relaunches at once instead of waiting for the stream to drain.  The life
// bound (0.8 ms by default) is what a device-wide synchronisation elsewhere in the process can wait.
template <int WT, class Eval>
__device__ __forceinline__ void sdf_server_loop(SdfMbox* mb, const long long idle, const long long life,
                                                const unsigned long long epoch, float* s_in, float* s_out,
                                                const int LH, const int max_rows, Eval&& eval) {
    __shared__ unsigned long long s_seq;
    __shared__ int s_go, s_rows, s_grad;
    const long long t0 = wall_clock64();
    long long last = t0;
    unsigned long long done = 0;
    if (threadIdx.x == 0) done = mb_load(&mb->seq_out);
    for (;;) {
        if (threadIdx.x == 0) {
            int go = 0;
            unsigned long long q = done;
            for (;;) {
                q = mb_load(&mb->seq_in);
                if (q != done) {
                    go = 1;
                    break;
                }
                const long long now = wall_clock64();
                if (mb_load(&mb->stop) || now - last > idle || now - t0 > life) break;
                __builtin_amdgcn_s_sleep(2);
            }
            s_go = go;
            s_seq = q;
            if (go) {
                const int rows = (int)mb_load_u32((const unsigned int*)&mb->rows);
                s_rows = rows < 1 ? 1 : (rows > max_rows ? max_rows : rows);
                s_grad = (int)mb_load_u32((const unsigned int*)&mb->grad);
            }
        }
        __syncthreads();
        if (!s_go) {
            if (threadIdx.x == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&mb->gone, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            break;
        }
        const long long t_seen = wall_clock64();
        const int rows = s_rows;
        for (int i = threadIdx.x; i < rows * (4 + LH); i += WT)
            s_in[i] = __uint_as_float(mb_load_u32((const unsigned int*)mb->in + i));
        __syncthreads();
        const long long t_staged = wall_clock64();
        eval(rows, s_grad);  // results go to LDS first, then to the mailbox with write-through stores
        const long long t_done = wall_clock64();
        // Publishing without an L2 write-back (__threadfence_system's buffer_wbl2, ~1.7 us each): the
        // results leave with system-scope stores, which write through the GPU caches to host memory; once
        // every wave's stores have completed (vmcnt(0)) and met at the barrier, one lane stores seq_out.
        // (Plain stores would stay in the L2 and the host would read stale results.)
        for (int i = threadIdx.x; i < rows * (s_grad ? 4 + LH : 4); i += WT)
            __hip_atomic_store((unsigned int*)mb->out + i, __float_as_uint(s_out[i]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            mb_store(&mb->t_seen, t_seen);
            mb_store(&mb->t_staged, t_staged);
            mb_store(&mb->t_done, t_done);
            mb_store(&mb->t_phase[13], t_done);  // closes the evaluators' phase stamps (t_phase[0..12], if any)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(&mb->seq_out, s_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            done = s_seq;
        }
        last = wall_clock64();
    }
}

}  // namespace sdfn
