// Ground truth from range images (csrc/df_truth.hip): the collision check of the reference's
// utils/collision_checker.py and the unsigned / signed distance fields of utils/df_computer.py.  fp32
// throughout, as the reference's Warp kernels (wp.float32).
#pragma once
#include <hip/hip_runtime.h>

namespace sdfn {

// the image model shared by the three computations (collision_checker.py:25-28, df_computer.py:87-88)
struct DfImg {
    const float* img;   // [n_img][H][W], normalised by dmax
    int n_img, H, W;
    float dmax, hfov, vfov;
    int is_depth, is_spherical;
    const float* points;  // [n][3]
    const int* p_to_i;    // [n] or nullptr: point j -> image j / per_img
    long long n, per_img; // per_img = n / n_img (used when p_to_i is nullptr)
};

struct ColcheckArgs {
    DfImg im;
    int outside;        // 0 free, 1 col, 2 extrapolate
    float safe_ball;
    unsigned char* out; // [n]
};

struct MinpoolArgs {
    const float* img;   // [n_img][H][W]
    float* out;         // [n_img][H/5][W/5]
    int n_img, H, W;
    float dmax;
};

struct UdfArgs {
    DfImg im;           // img = the pooled images, H, W = the pooled sizes
    float max_df;
    float* udf;         // [n]
    float* grad;        // [n][3]
    int* pix_idx;       // [n] or nullptr
};

struct SdfGridArgs {
    DfImg im;
    float min_df, max_df;
    const float* grid;  // [G][3]
    const float* dist;  // [G]
    const int* orig_idx;  // [G] (the grid is sorted by dist, ascending) or nullptr (any order, full scan)
    int G;
    float* sdf;         // [n]
    float* grad;        // [n][3]
    int* vox_idx;       // [n] or nullptr; -1 where no voxel counts
};

constexpr int DF_BLOCK = 256;
// LDS of udf_kernel: (cos, sin) or tan per pooled column and row
inline size_t udf_lds_bytes(int h, int w) { return (size_t)2 * ((size_t)h + (size_t)w) * sizeof(float); }
constexpr size_t UDF_LDS_MAX = 48 * 1024;

hipError_t launch_colcheck(const ColcheckArgs& a, hipStream_t s);
hipError_t launch_minpool5(const MinpoolArgs& a, hipStream_t s);
hipError_t launch_udf(const UdfArgs& a, hipStream_t s);
hipError_t launch_sdf_grid(const SdfGridArgs& a, hipStream_t s);

}  // namespace sdfn
