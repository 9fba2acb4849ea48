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

// udf_kernel / sdf_grid_kernel as the image field's rows kernel (x != nullptr): point pt is node row pt
struct DfRowsArgs {
    const double* x;    // [rows][10]
    const double* p;    // [rows][np]
    double* h;          // [rows][3]: column 2 is written
    double* Jh;         // [rows][10][3]: column 2 is written
    float* pts;         // [rows][3], == the kernel's im.points: written by the kernel, then read by its scan
    const int* img_of;  // [B] or nullptr
    int N1, np;
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

// launch_img_sdf_rows: the field of sdf_grid_kernel (is_signed) or udf_kernel at the node rows of a batch, as the SDF
// row of h / J_h
struct ImgSdfArgs {
    const float* images;  // [n_img][H][W], normalised by dmax (signed)
    const float* pooled;  // [n_img][H/5][W/5], the min-pooled images (unsigned)
    const int* img_of;    // [B] or nullptr: instance b -> image b
    int H, W;             // of the images (the pooled size is H / 5, W / 5)
    float dmax, hfov, vfov;
    int is_depth, is_spherical;
    int is_signed;
    float min_df, max_df;
    const float* grid;    // signed: as SdfGridArgs
    const float* dist;
    const int* orig_idx;
    int G;
    long long rows;       // B (N+1)
    int N1, np;           // nodes per instance, parameters per node
    const double* x;      // [rows][10]: the world position is x[r][0:3]
    const double* p;      // [rows][np]: flag p[r][0], W_p_Co p[r][1:4], W_R_Co p[r][4:13] row-major
    double* h;            // [rows][3]: column 2 is written
    double* Jh;           // [rows][10][3]: column 2 is written
    float* pts;           // [rows][3]: the camera-frame point of every row (required at the launch)
};

constexpr int DF_BLOCK = 256;
// LDS of udf_kernel: (cos, sin) or tan per pooled column and row
inline size_t udf_lds_bytes(int h, int w) { return (size_t)2 * ((size_t)h + (size_t)w) * sizeof(float); }
constexpr size_t UDF_LDS_MAX = 48 * 1024;

hipError_t launch_colcheck(const ColcheckArgs& a, hipStream_t s);
hipError_t launch_minpool5(const MinpoolArgs& a, hipStream_t s);
hipError_t launch_udf(const UdfArgs& a, hipStream_t s);
hipError_t launch_sdf_grid(const SdfGridArgs& a, hipStream_t s);
hipError_t launch_img_sdf_rows(const ImgSdfArgs& a, hipStream_t s);

}  // namespace sdfn
