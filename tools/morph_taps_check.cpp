// Stand-alone host check of the morphology tap-list builder (csrc/morph_taps.h), meant to be built with a sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o tools/_morph_taps_check tools/morph_taps_check.cpp && tools/_morph_taps_check
//
// It builds the lists of both operations for the elements of tests/golden/preproc_golden.npz (3 x 3 of ones, the
// asymmetric 4 x 3 element, the discs of radius 3 and 10), the 1 x 1 element, single rows and columns of the largest
// size, an element without a 1 and out-of-range sizes, with the element in a heap block of exactly k_h k_w bytes and
// the list between guard words, and checks every list against its definition.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdf-nmpc_amd/csrc/morph_taps.h"

using namespace sdfn;

static int failures = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static void check(const char* name, const std::vector<unsigned char>& el, int k_h, int k_w) {
    unsigned char* heap = (unsigned char*)std::malloc(el.size());  // exactly k_h k_w bytes: an overrun is seen
    std::memcpy(heap, el.data(), el.size());
    int ones = 0;
    for (unsigned char v : el) ones += v != 0;
    for (int op = 0; op < 2; ++op) {
        struct { unsigned guard0; MorphTaps t; unsigned guard1; } g;
        g.guard0 = g.guard1 = 0xA5A5A5A5u;
        std::memset(&g.t, 0xFF, sizeof(g.t));
        const int n = morph_build_taps(op, heap, k_h, k_w, &g.t);
        CHECK(g.guard0 == 0xA5A5A5A5u && g.guard1 == 0xA5A5A5A5u);
        CHECK(n == ones && g.t.n == ones && g.t.n_all == k_h * k_w);
        const int lw = MORPH_TILE + k_w - 1;
        std::vector<int> seen(k_h * k_w, 0);
        for (int t = 0; t < g.t.n_all; ++t) {
            const int i = g.t.off[t] / lw, j = g.t.off[t] % lw;
            CHECK(i < k_h && j < k_w);
            if (i >= k_h || j >= k_w) continue;
            CHECK(g.t.off[t] + (MORPH_TILE - 1) * lw + MORPH_TILE - 1 < (MORPH_TILE + k_h - 1) * lw);  // inside the LDS tile
            const int e = op == MORPH_DILATE ? (k_h - 1 - i) * k_w + (k_w - 1 - j) : i * k_w + j;
            CHECK((el[e] != 0) == (t < g.t.n));  // included taps first, of the flipped element for a dilation
            ++seen[i * k_w + j];
        }
        for (int v : seen) CHECK(v == 1);
    }
    std::free(heap);
    std::printf("%-10s %2d x %2d: %3d of %3d taps included\n", name, k_h, k_w, ones, k_h * k_w);
}

static std::vector<unsigned char> disc(int r) {
    std::vector<unsigned char> d((2 * r + 1) * (2 * r + 1));
    for (int i = -r; i <= r; ++i)
        for (int j = -r; j <= r; ++j) d[(i + r) * (2 * r + 1) + j + r] = i * i + j * j <= r * r;
    return d;
}

int main() {
    check("ones3", std::vector<unsigned char>(9, 1), 3, 3);
    check("asym", {1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1}, 4, 3);
    check("disc3", disc(3), 7, 7);
    check("disc10", disc(10), 21, 21);
    check("one", {1}, 1, 1);
    check("row21", std::vector<unsigned char>(21, 1), 1, 21);
    check("col21", std::vector<unsigned char>(21, 1), 21, 1);
    check("ones21", std::vector<unsigned char>(441, 1), 21, 21);
    check("empty", std::vector<unsigned char>(9, 0), 3, 3);  // n == 0: the entry point refuses it
    MorphTaps t;
    unsigned char one = 1;
    CHECK(morph_build_taps(0, &one, 0, 1, &t) == -1 && morph_build_taps(0, &one, 1, 22, &t) == -1);
    CHECK(morph_build_taps(2, &one, 1, 1, &t) == -1 && morph_build_taps(0, nullptr, 1, 1, &t) == -1);
    CHECK(morph_build_taps(1, &one, 1, 1, nullptr) == -1);
    std::printf(failures ? "%d checks FAILED\n" : "all checks passed\n", failures);
    return failures != 0;
}
