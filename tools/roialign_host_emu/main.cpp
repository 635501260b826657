// Host emulation of skg_roialign.hip: the kernels run on the CPU, one host thread per work-item (hip/hip_runtime.h here is a
// stand-in for the HIP runtime), so that AddressSanitizer / UBSan see every map, output and LDS-tile access.  Compares the
// channels-last entries against the [B, C, H, W] entries on the same values: forward outputs byte for byte (nine dtype
// pairs), fp32 gradients within 2e-5.  Shapes and boxes of tests/test_half_features_gpu.py::_roi_inputs.  No GPU involved.
//
//   cd tools/roialign_host_emu && clang++ -x c++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread \
//       -I. -I../../skghoi_amd/csrc -I../../include main.cpp -o emu && ./emu        (a few minutes: 256 threads per workgroup)
// Exit status 0 and "bad 0" on the last line: everything agreed.
#include "skg_roialign.hip"
#include <cstdio>
#include <cstdlib>
#include <random>
thread_local dim3 threadIdx, blockIdx, gridDim;
std::barrier<>* g_barrier;

static uint16_t to_bf16(float v) { uint32_t u = __float_as_uint(v); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }

template <class T> static T conv(float v);
template <> float conv<float>(float v) { return v; }
template <> _Float16 conv<_Float16>(float v) { return (_Float16)v; }
template <> uint16_t conv<uint16_t>(float v) { return to_bf16(v); }

static const float BOXES[8][4] = {{10.3f, 20.1f, 150.7f, 180.2f}, {0.f, 0.f, 319.f, 199.f}, {100.f, 50.f, 104.f, 53.f},
                                  {250.f, 10.f, 318.f, 60.f}, {5.f, 5.f, 5.5f, 5.2f}, {30.f, 40.f, 90.f, 160.f},
                                  {-5.f, -3.f, 40.f, 30.f}, {200.f, 150.f, 330.f, 210.f}};
static const int IMG[8] = {0, 0, 0, 0, 0, 1, 1, 1};

template <class T>
static int run(int map_dt, int Cc, int L0, int L, int pooled, int sampling) {
    const int B = 2;
    std::mt19937 rng(Cc * 7 + map_dt);
    std::normal_distribution<float> nd;
    std::vector<T*> nchw(L), nhwc(L);
    std::vector<float*> g_nchw(L), g_nhwc(L);
    int32_t H[8], W[8]; float sc[8];
    for (int l = 0; l < L; ++l) {
        const int s = 4 << (l + L0);
        H[l] = 200 / s; W[l] = 320 / s; sc[l] = 1.f / s;
        const size_t n = (size_t)B * Cc * H[l] * W[l];
        nchw[l] = (T*)aligned_alloc(16, n * sizeof(T)); nhwc[l] = (T*)aligned_alloc(16, n * sizeof(T));
        g_nchw[l] = (float*)aligned_alloc(16, n * 4); g_nhwc[l] = (float*)aligned_alloc(16, n * 4);
        memset(g_nchw[l], 0, n * 4); memset(g_nhwc[l], 0, n * 4);
        for (int b = 0; b < B; ++b) for (int c = 0; c < Cc; ++c) for (int y = 0; y < H[l]; ++y) for (int x = 0; x < W[l]; ++x) {
            const T v = conv<T>(nd(rng));
            nchw[l][(((size_t)b * Cc + c) * H[l] + y) * W[l] + x] = v;
            nhwc[l][(((size_t)b * H[l] + y) * W[l] + x) * Cc + c] = v;
        }
    }
    float* boxes = (float*)aligned_alloc(16, 8 * 16); memcpy(boxes, BOXES, 8 * 16);
    int32_t* img = (int32_t*)aligned_alloc(16, 32); memcpy(img, IMG, 32);
    const int kmin = L > 1 ? 2 + L0 : 0, kmax = L > 1 ? kmin + L - 1 : 0;
    const size_t no = (size_t)8 * Cc * pooled * pooled;
    int bad = 0;
    for (int odt = 0; odt < 3; ++odt) {
        const size_t es = odt == 0 ? 4 : 2;
        void* o1 = aligned_alloc(16, (no * es + 15) / 16 * 16); void* o2 = aligned_alloc(16, (no * es + 15) / 16 * 16);
        memset(o1, 0xAB, no * es); memset(o2, 0xCD, no * es);
        int r1 = skg_roi_align_x((const void* const*)nchw.data(), map_dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, 8, pooled, sampling, o1, odt, nullptr);
        int r2 = skg_roi_align_nhwc_x((const void* const*)nhwc.data(), map_dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, 8, pooled, sampling, o2, odt, nullptr);
        if (r1 || r2 || memcmp(o1, o2, no * es)) { printf("  MISMATCH fwd mdt %d odt %d C %d L %d pooled %d samp %d rc %d %d\n", map_dt, odt, Cc, L, pooled, sampling, r1, r2); ++bad; }
        free(o1); free(o2);
    }
    if (map_dt == 0) {
        float* dout = (float*)aligned_alloc(16, (no * 4 + 15) / 16 * 16);
        for (size_t i = 0; i < no; ++i) dout[i] = nd(rng);
        int r1 = skg_roi_align_bwd_f32(g_nchw.data(), H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, 8, pooled, sampling, dout, nullptr);
        int r2 = skg_roi_align_bwd_nhwc_f32(g_nhwc.data(), H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, 8, pooled, sampling, dout, nullptr);
        double worst = 0, mass = 0;
        for (int l = 0; l < L; ++l)
            for (int b = 0; b < B; ++b) for (int c = 0; c < Cc; ++c) for (int y = 0; y < H[l]; ++y) for (int x = 0; x < W[l]; ++x) {
                const float a = g_nchw[l][(((size_t)b * Cc + c) * H[l] + y) * W[l] + x];
                const float d = g_nhwc[l][(((size_t)b * H[l] + y) * W[l] + x) * Cc + c];
                worst = fmax(worst, fabs((double)a - d)); mass += fabs(a);
            }
        printf("  bwd C %d L %d pooled %d samp %d: rc %d %d, max diff %.3e, sum|g| %.1f\n", Cc, L, pooled, sampling, r1, r2, worst, mass);
        if (r1 || r2 || worst > 2e-5 || mass == 0) ++bad;
        free(dout);
    }
    for (int l = 0; l < L; ++l) { free(nchw[l]); free(nhwc[l]); free(g_nchw[l]); free(g_nhwc[l]); }
    free(boxes); free(img);
    return bad;
}

int main() {
    int bad = 0;
    const int Cs[3] = {8, 24, 72};
    for (int ci = 0; ci < 3; ++ci) {
        const int Cc = Cs[ci];
        const int cfg[4][4] = {{0, 4, 7, 2}, {3, 1, 7, 2}, {0, 4, 7, 0}, {0, 4, 2, 2}};
        for (int k = 0; k < 4; ++k) {
            if (ci == 2 && k > 0 && k != 2) continue;
            printf("C %d cfg %d\n", Cc, k);
            bad += run<float>(0, Cc, cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3]);
            bad += run<_Float16>(1, Cc, cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3]);
            bad += run<uint16_t>(2, Cc, cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3]);
        }
    }
    int64_t cnt[4]; skg_roi_align_layout_counts(cnt, 1);
    printf("counts %lld %lld %lld %lld, bad %d\n", (long long)cnt[0], (long long)cnt[1], (long long)cnt[2], (long long)cnt[3], bad);
    return bad != 0;
}
