// The tap list of a morphological launch (csrc/morph.hip), built on the host at call time.  Plain C++ without a
// HIP include, so that the builder can be compiled into a stand-alone host program and run under a sanitizer
// (tools/morph_taps_check.cpp).
//
// The reference's Dilate / Erode (utils/preprocessing.py:100-199) pad the image by origin = (k_h / 2, k_w / 2) on
// the top / left and k - origin - 1 on the bottom / right, and scan channel (i, j) = padded[y + i][x + j] + bias(i, j).
// Erode's bias is 0 where the element is 1 and +2 where it is 0; Dilate's bias (0 / -2) is that mask *flipped*
// (mask.flip(0) of the flattened element) over the unflipped padding: tap (i, j) is included where
// element[k_h-1-i][k_w-1-j] is 1.  An excluded tap is not skipped: it enters the min / max with its bias, and wins
// where every included tap reads the border value (padding, or a zero under ignore_zeros) and the excluded pixel
// does not -- so the list carries the included taps first and the excluded ones after them.
#pragma once

namespace sdfn {

constexpr int MORPH_K_MAX = 21;   // the reference's disc of radius 10
constexpr int MORPH_TILE = 16;    // output pixels per block: MORPH_TILE x MORPH_TILE, one per lane
constexpr int MORPH_LDS_W = MORPH_TILE + MORPH_K_MAX - 1;
constexpr int MORPH_DILATE = 0, MORPH_ERODE = 1;

struct MorphTaps {
    int n;                                         // included taps, >= 1: off[0..n)
    int n_all;                                     // k_h * k_w: the excluded taps are off[n..n_all)
    unsigned short off[MORPH_K_MAX * MORPH_K_MAX];  // i * (MORPH_TILE + k_w - 1) + j: the tap's offset in the LDS tile
};

// element [k_h][k_w], row-major, a tap is included where the entry is not 0.  Returns the number of included taps,
// 0 for an element without a 1 (the caller refuses it), -1 for bad arguments; both parts of out->off in scan order.
inline int morph_build_taps(int op, const unsigned char* element, int k_h, int k_w, MorphTaps* out) {
    if (!element || !out || (op != MORPH_DILATE && op != MORPH_ERODE)) return -1;
    if (k_h < 1 || k_h > MORPH_K_MAX || k_w < 1 || k_w > MORPH_K_MAX) return -1;
    const int lw = MORPH_TILE + k_w - 1;
    int n = 0;
    for (int pass = 0; pass < 2; ++pass) {  // the included taps, then the excluded ones
        for (int i = 0; i < k_h; ++i)
            for (int j = 0; j < k_w; ++j) {
                const int e = op == MORPH_DILATE ? (k_h - 1 - i) * k_w + (k_w - 1 - j) : i * k_w + j;
                if ((element[e] != 0) == (pass == 0)) out->off[n++] = (unsigned short)(i * lw + j);
            }
        if (pass == 0) out->n = n;
    }
    out->n_all = n;
    return out->n;
}

}  // namespace sdfn
