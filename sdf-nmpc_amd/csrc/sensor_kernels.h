// Image morphology (csrc/morph.hip) and the sensor-degradation stage (csrc/sensor.hip): what stands between the
// renderer (scene.hip) or a real depth camera and the consumers of an image (vae_enc.hip, df_truth.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "morph_taps.h"

namespace sdfn {

constexpr int MORPH_BLOCK = MORPH_TILE * MORPH_TILE;  // 256: four wavefronts
constexpr int SENSOR_BLOCK = 256;
constexpr int SENSOR_MAX_BOXES = 8;

struct MorphArgs {
    const float* in;   // [B][H][W]
    float* out;        // [B][H][W], != in
    int B, H, W;
    int k_h, k_w, oh, ow;  // element size and origin (k_h / 2, k_w / 2)
    int op, ignore_zeros;
    float border;      // -2 (dilate) / +2 (erode)
    MorphTaps taps;
};

struct OutlierArgs {
    const float* in;   // [B][H][W]
    float* out;        // [B][H][W], != in
    int B, H, W;
    float min_range;
};

struct SensorArgs {
    float* img;        // [B][H][W], in place
    int B, H, W;
    unsigned key0, key1;   // the seed's low and high words
    unsigned frame;
    float a, b, vmax;
    unsigned p_thresh;
    int miss_invalid;
    const int16_t* boxes;  // [n_frames][B][max_boxes][4] (y0, x0, h, w) or nullptr
    int n_frames, max_boxes;
    const int* stream_id;  // [B] or nullptr (b)
};

hipError_t launch_morph(const MorphArgs& a, hipStream_t s);
hipError_t launch_outlier_rm(const OutlierArgs& a, hipStream_t s);
// the pieces of RemoveCloseOutliers with kernel_size != 3: out = in < min_range ? 0 : in, and
// img = img > 0 ? t : img
hipError_t launch_morph_threshold(const float* in, float* out, long long n, float min_range, hipStream_t s);
hipError_t launch_morph_restore(float* img, const float* t, long long n, hipStream_t s);
hipError_t launch_sensor_degrade(const SensorArgs& a, hipStream_t s);

}  // namespace sdfn
