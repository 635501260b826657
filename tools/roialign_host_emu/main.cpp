// Host emulation of skg_roialign.hip: the kernels run on the CPU, one host thread per work-item (hip/hip_runtime.h here is a
// stand-in for the HIP runtime), so that AddressSanitizer / UBSan see every map, output and LDS-tile access.  Compares the
// channels-last entries against the [B, C, H, W] entries on the same values: forward outputs byte for byte (nine dtype
// pairs), fp32 gradients within 2e-5; and the two deterministic backward kernels byte for byte against a sequential loop
// written here (run_det below).  Every case prints FNV-1a digests of its forward outputs / deterministic gradients: the
// logs of two builds (-I a directory holding another skg_roialign.hip first) must agree line for line.  Shapes and boxes
// of tests/test_half_features_gpu.py::_roi_inputs.  No GPU involved.
//
//   cd tools/roialign_host_emu && clang++ -x c++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread \
//       -I. -I../../skghoi_amd/csrc -I../../include main.cpp -o emu && ./emu        (a few minutes: 256 threads per workgroup)
// Exit status 0 and "bad 0" on the last line: everything agreed.  `./emu det` runs the deterministic backward part alone,
// `./emu mirror` the mirrored entries alone (run_mirror below: against the plain entries on maps mirrored here).
#include "skg_roialign.hip"
#include <cstdio>
#include <cstdlib>
#include <random>
thread_local dim3 threadIdx, blockIdx, gridDim;
std::barrier<>* g_barrier;

// 64-bit FNV-1a over a buffer (chained through h): printed per case, so that two builds of the kernels can be compared
static uint64_t fnv1a(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 0x100000001b3ull;
    return h;
}

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
    unsigned long long dig[2][3];
    for (int odt = 0; odt < 3; ++odt) {
        const size_t es = odt == 0 ? 4 : 2;
        void* o1 = aligned_alloc(16, (no * es + 15) / 16 * 16); void* o2 = aligned_alloc(16, (no * es + 15) / 16 * 16);
        memset(o1, 0xAB, no * es); memset(o2, 0xCD, no * es);
        int r1 = skg_roi_align_x((const void* const*)nchw.data(), map_dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, 8, pooled, sampling, o1, odt, nullptr);
        int r2 = skg_roi_align_nhwc_x((const void* const*)nhwc.data(), map_dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, 8, pooled, sampling, o2, odt, nullptr);
        if (r1 || r2 || memcmp(o1, o2, no * es)) { printf("  MISMATCH fwd mdt %d odt %d C %d L %d pooled %d samp %d rc %d %d\n", map_dt, odt, Cc, L, pooled, sampling, r1, r2); ++bad; }
        dig[0][odt] = fnv1a(o1, no * es); dig[1][odt] = fnv1a(o2, no * es);
        free(o1); free(o2);
    }
    printf("  fwd mdt %d C %d L %d pooled %d samp %d: digests %016llx %016llx %016llx, channels-last %016llx %016llx %016llx\n", map_dt,
           Cc, L, pooled, sampling, dig[0][0], dig[0][1], dig[0][2], dig[1][0], dig[1][1], dig[1][2]);
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


// ---------------------------------------------------------------------------------------- deterministic backward
// skg_roi_align_bwd_det_x / skg_roi_align_bwd_det_nhwc_x against a plain sequential loop that applies the contract's order:
// RoIs ascending, sample rows then sample columns ascending, taps 1..4, fp32 `acc += (wy * wx) * (dout / cnt)` from 0.f (a
// sequential scatter gives every element its terms in exactly that order), rounded once.  Byte for byte, both layouts, maps
// prefilled with 0xFF bytes (NaN), three images of which image 1 has no boxes.
static const float DBOX[12][4] = {{10.f, 15.f, 60.f, 70.f}, {20.f, 20.f, 70.f, 65.f}, {10.f, 15.f, 60.f, 70.f},
                                  {5.3f, 8.1f, 150.7f, 140.2f}, {0.f, 0.f, 179.f, 119.f}, {-60.f, -50.f, 240.f, 170.f},
                                  {-300.f, -250.f, 500.f, 400.f}, {50.f, 30.f, 52.f, 31.5f}, {3.f, 3.f, 3.4f, 3.2f},
                                  {150.f, 90.f, 200.f, 130.f}, {30.f, 40.f, 90.f, 110.f}, {100.f, 60.f, 179.f, 119.f}};
static const int DIMG[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2};

static void det_reference(std::vector<std::vector<float>>& g, const int32_t* H, const int32_t* W, const float* sc, int L,
                          int Cc, int kmin, int kmax, const float* boxes, const int* img, int n_rois, int B, int pooled,
                          int sampling, const float* dout, std::vector<int>& level_used) {
    for (int r = 0; r < n_rois; ++r) {
        const float* b = boxes + 4 * r;
        if (img[r] < 0 || img[r] >= B) continue;
        const float s = sqrtf((b[2] - b[0]) * (b[3] - b[1]));
        float lv = floorf((float)4 + log2f(s / 224.f) + 1e-6f);
        lv = fminf(fmaxf(lv, (float)kmin), (float)kmax);
        const int l = (int)lv - kmin;
        level_used[l]++;
        const int Hl = H[l], Wl = W[l];
        const float x1 = b[0] * sc[l], y1 = b[1] * sc[l], x2 = b[2] * sc[l], y2 = b[3] * sc[l];
        const float rw = fmaxf(x2 - x1, 1.f), rh = fmaxf(y2 - y1, 1.f);
        const float bw = rw / (float)pooled, bh = rh / (float)pooled;
        const int gh = sampling > 0 ? sampling : (int)ceilf(rh / pooled);
        const int gw = sampling > 0 ? sampling : (int)ceilf(rw / pooled);
        const float cnt = fmaxf((float)(gh * gw), 1.f);
        for (int c = 0; c < Cc; ++c) {
            float* f = g[l].data() + ((size_t)img[r] * Cc + c) * Hl * Wl;
            for (int sy = 0; sy < pooled * gh; ++sy) for (int sx = 0; sx < pooled * gw; ++sx) {
                const int ph = sy / gh, iy = sy % gh, pw = sx / gw, ix = sx % gw;
                float y = y1 + ph * bh + (iy + 0.5f) * bh / (float)gh;
                float x = x1 + pw * bw + (ix + 0.5f) * bw / (float)gw;
                if (y < -1.0f || y > (float)Hl || x < -1.0f || x > (float)Wl) continue;
                if (y <= 0.f) y = 0.f;
                if (x <= 0.f) x = 0.f;
                int yl = (int)y, xl = (int)x, yh, xh;
                if (yl >= Hl - 1) { yh = yl = Hl - 1; y = (float)yl; } else yh = yl + 1;
                if (xl >= Wl - 1) { xh = xl = Wl - 1; x = (float)xl; } else xh = xl + 1;
                const float ly = y - yl, lx = x - xl, hy = 1.f - ly, hx = 1.f - lx;
                const float gr = dout[(((size_t)r * Cc + c) * pooled + ph) * pooled + pw] / cnt;
                f[yl * Wl + xl] += (hy * hx) * gr;
                f[yl * Wl + xh] += (hy * lx) * gr;
                f[yh * Wl + xl] += (ly * hx) * gr;
                f[yh * Wl + xh] += (ly * lx) * gr;
            }
        }
    }
}

template <class T> static T conv_nan(float v) { return conv<T>(v); }
template <> uint16_t conv_nan<uint16_t>(float v) { return v != v ? (uint16_t)0x7FC0 : to_bf16(v); }

template <class T>
static int run_det(int dt, int Cc, int L0, int L, int pooled, int sampling, int n_rois, int far_image) {
    const int B = 3;
    std::mt19937 rng(Cc * 11 + dt);
    std::normal_distribution<float> nd;
    int32_t H[8], W[8]; float sc[8];
    std::vector<T*> g_nchw(L), g_nhwc(L);
    std::vector<std::vector<float>> ref(L);
    for (int l = 0; l < L; ++l) {
        const int s = 4 << (l + L0);
        H[l] = 120 / s; W[l] = 180 / s; sc[l] = 1.f / s;
        const size_t n = (size_t)B * Cc * H[l] * W[l];
        g_nchw[l] = (T*)aligned_alloc(16, (n * sizeof(T) + 15) / 16 * 16); g_nhwc[l] = (T*)aligned_alloc(16, (n * sizeof(T) + 15) / 16 * 16);
        memset(g_nchw[l], 0xFF, n * sizeof(T)); memset(g_nhwc[l], 0xFF, n * sizeof(T));
        ref[l].assign(n, 0.f);
    }
    float* boxes = (float*)aligned_alloc(16, 12 * 16); memcpy(boxes, DBOX, 12 * 16);
    int32_t* img = (int32_t*)aligned_alloc(16, 48); memcpy(img, DIMG, 48);
    if (far_image) img[n_rois - 1] = 7;                                // a RoI of an image that does not exist
    const int kmin = L > 1 ? 2 + L0 : 0, kmax = L > 1 ? kmin + L - 1 : 0;
    const size_t no = (size_t)12 * Cc * pooled * pooled;
    float* dout = (float*)aligned_alloc(16, (no * 4 + 15) / 16 * 16);
    for (size_t i = 0; i < no; ++i) dout[i] = nd(rng);
    std::vector<int> used(L, 0);
    det_reference(ref, H, W, sc, L, Cc, kmin, kmax, boxes, img, n_rois, B, pooled, sampling, dout, used);
    const int r1 = skg_roi_align_bwd_det_x((void* const*)g_nchw.data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, n_rois, B, pooled, sampling, dout, nullptr);
    const int r2 = skg_roi_align_bwd_det_nhwc_x((void* const*)g_nhwc.data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, n_rois, B, pooled, sampling, dout, nullptr);
    size_t d1 = 0, d2 = 0, nonzero = 0, img1 = 0;
    for (int l = 0; l < L; ++l)
        for (int b = 0; b < B; ++b) for (int c = 0; c < Cc; ++c) for (int y = 0; y < H[l]; ++y) for (int x = 0; x < W[l]; ++x) {
            const float rv = ref[l][(((size_t)b * Cc + c) * H[l] + y) * W[l] + x];
            const T want = conv_nan<T>(rv);
            d1 += memcmp(&want, &g_nchw[l][(((size_t)b * Cc + c) * H[l] + y) * W[l] + x], sizeof(T)) != 0;
            d2 += memcmp(&want, &g_nhwc[l][(((size_t)b * H[l] + y) * W[l] + x) * Cc + c], sizeof(T)) != 0;
            nonzero += rv != 0.f; img1 += b == 1 && rv != 0.f;
        }
    int levels = 0;
    uint64_t h1 = fnv1a(nullptr, 0), h2 = h1;
    for (int l = 0; l < L; ++l) {
        levels += used[l] > 0;
        const size_t n = (size_t)B * Cc * H[l] * W[l] * sizeof(T);
        h1 = fnv1a(g_nchw[l], n, h1); h2 = fnv1a(g_nhwc[l], n, h2);
    }
    printf("  det dt %d C %d L %d pooled %d samp %d rois %d far %d: rc %d %d, differing elements %zu %zu, nonzero %zu, levels used %d, digests %016llx %016llx\n",
           dt, Cc, L, pooled, sampling, n_rois, far_image, r1, r2, d1, d2, nonzero, levels, (unsigned long long)h1, (unsigned long long)h2);
    const bool covered = n_rois == 0 ? nonzero == 0 : (nonzero > 0 && levels == L);
    for (int l = 0; l < L; ++l) { free(g_nchw[l]); free(g_nhwc[l]); }
    free(boxes); free(img); free(dout);
    return (r1 || r2 || d1 || d2 || img1 || !covered) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------- mirrored images
// The *_mirror_* entries with flags {1, 0, 1} on three images (image 1 has no boxes) against the plain entries on copies of
// the maps whose flagged images are mirrored along W: forward outputs byte for byte, deterministic gradients byte for byte
// against the plain deterministic gradients mirrored back, both layouts, maps prefilled with 0xFF bytes; fp32 atomics within
// 2e-5 of the deterministic mirrored gradients.  The boxes of DBOX cross and leave both edges, so the sanitizers see every
// mirrored address.
template <class T>
static int run_mirror(int dt, int Cc, int L0, int L, int pooled, int sampling) {
    const int B = 3, R = 12;
    const int32_t flags_h[3] = {1, 0, 1};
    std::mt19937 rng(Cc * 13 + dt);
    std::normal_distribution<float> nd;
    int32_t H[8], W[8]; float sc[8];
    std::vector<T*> m[2], mf[2], g[2], gf[2];                          // [layout]: maps, mirrored copies, gradients of both routes
    std::vector<float*> ga[2];                                         // fp32 atomics gradients
    for (int k = 0; k < 2; ++k) { m[k].resize(L); mf[k].resize(L); g[k].resize(L); gf[k].resize(L); ga[k].resize(L); }
    auto at = [&](int k, int l, int b, int c, int y, int x) {
        return k == 0 ? (((size_t)b * Cc + c) * H[l] + y) * W[l] + x : (((size_t)b * H[l] + y) * W[l] + x) * Cc + c;
    };
    for (int l = 0; l < L; ++l) {
        const int s = 4 << (l + L0);
        H[l] = 120 / s; W[l] = 180 / s; sc[l] = 1.f / s;
        const size_t n = (size_t)B * Cc * H[l] * W[l], bytes = (n * sizeof(T) + 15) / 16 * 16;
        for (int k = 0; k < 2; ++k) {
            m[k][l] = (T*)aligned_alloc(16, bytes); mf[k][l] = (T*)aligned_alloc(16, bytes);
            g[k][l] = (T*)aligned_alloc(16, bytes); gf[k][l] = (T*)aligned_alloc(16, bytes);
            memset(g[k][l], 0xFF, n * sizeof(T)); memset(gf[k][l], 0xFF, n * sizeof(T));
            ga[k][l] = (float*)aligned_alloc(16, (n * 4 + 15) / 16 * 16); memset(ga[k][l], 0, n * 4);
        }
        for (int b = 0; b < B; ++b) for (int c = 0; c < Cc; ++c) for (int y = 0; y < H[l]; ++y) for (int x = 0; x < W[l]; ++x) {
            const T v = conv<T>(nd(rng));
            const int xf = flags_h[b] ? W[l] - 1 - x : x;
            for (int k = 0; k < 2; ++k) { m[k][l][at(k, l, b, c, y, x)] = v; mf[k][l][at(k, l, b, c, y, xf)] = v; }
        }
    }
    float* boxes = (float*)aligned_alloc(16, R * 16); memcpy(boxes, DBOX, R * 16);
    int32_t* img = (int32_t*)aligned_alloc(16, 48); memcpy(img, DIMG, 48);
    int32_t* flags = (int32_t*)aligned_alloc(16, 16); memcpy(flags, flags_h, 12);
    const int kmin = L > 1 ? 2 + L0 : 0, kmax = L > 1 ? kmin + L - 1 : 0;
    const size_t no = (size_t)R * Cc * pooled * pooled, ob = (no * sizeof(T) + 15) / 16 * 16;
    float* dout = (float*)aligned_alloc(16, (no * 4 + 15) / 16 * 16);
    for (size_t i = 0; i < no; ++i) dout[i] = nd(rng);
    int bad = 0, rc = 0;
    size_t fwd_diff = 0, fwd_same_as_plain = 0, det_diff = 0, nonzero = 0;
    double worst = 0;
    for (int k = 0; k < 2; ++k) {
        void* o1 = aligned_alloc(16, ob); void* o2 = aligned_alloc(16, ob); void* o3 = aligned_alloc(16, ob);
        memset(o1, 0xAB, no * sizeof(T)); memset(o2, 0xCD, no * sizeof(T)); memset(o3, 0xEF, no * sizeof(T));
        if (k == 0) {
            rc |= skg_roi_align_mirror_x((const void* const*)m[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, o1, dt, flags, B, nullptr);
            rc |= skg_roi_align_x((const void* const*)mf[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, o2, dt, nullptr);
            rc |= skg_roi_align_mirror_x((const void* const*)m[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, o3, dt, nullptr, 0, nullptr);
            rc |= skg_roi_align_bwd_det_mirror_x((void* const*)g[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, B, pooled, sampling, dout, flags, nullptr);
            rc |= skg_roi_align_bwd_det_x((void* const*)gf[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, B, pooled, sampling, dout, nullptr);
            if (dt == 0) rc |= skg_roi_align_bwd_mirror_f32(ga[k].data(), H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, dout, flags, B, nullptr);
        } else {
            rc |= skg_roi_align_mirror_nhwc_x((const void* const*)m[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, o1, dt, flags, B, nullptr);
            rc |= skg_roi_align_nhwc_x((const void* const*)mf[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, o2, dt, nullptr);
            rc |= skg_roi_align_mirror_nhwc_x((const void* const*)m[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, o3, dt, nullptr, 0, nullptr);
            rc |= skg_roi_align_bwd_det_mirror_nhwc_x((void* const*)g[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, B, pooled, sampling, dout, flags, nullptr);
            rc |= skg_roi_align_bwd_det_nhwc_x((void* const*)gf[k].data(), dt, H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, B, pooled, sampling, dout, nullptr);
            if (dt == 0) rc |= skg_roi_align_bwd_mirror_nhwc_f32(ga[k].data(), H, W, sc, L, Cc, kmin, kmax, 224.f, 4, boxes, img, R, pooled, sampling, dout, flags, B, nullptr);
        }
        fwd_diff += memcmp(o1, o2, no * sizeof(T)) != 0;
        fwd_same_as_plain += memcmp(o1, o3, no * sizeof(T)) == 0;      // (the flags must change something)
        for (int l = 0; l < L; ++l)
            for (int b = 0; b < B; ++b) for (int c = 0; c < Cc; ++c) for (int y = 0; y < H[l]; ++y) for (int x = 0; x < W[l]; ++x) {
                const int xf = flags_h[b] ? W[l] - 1 - x : x;
                const T a = g[k][l][at(k, l, b, c, y, x)], w = gf[k][l][at(k, l, b, c, y, xf)];
                det_diff += memcmp(&a, &w, sizeof(T)) != 0;
                det_diff += k == 1 && memcmp(&a, &g[0][l][at(0, l, b, c, y, x)], sizeof(T)) != 0;    // both layouts: the same bits
                if (dt == 0) {
                    float av; memcpy(&av, &a, 4);
                    worst = fmax(worst, fabs((double)av - ga[k][l][at(k, l, b, c, y, x)]));
                    nonzero += av != 0.f;
                }
            }
        free(o1); free(o2); free(o3);
    }
    printf("  mirror dt %d C %d L %d pooled %d samp %d: rc %d, forward buffers differing %zu (equal to the unflagged run %zu), "
           "deterministic elements differing %zu, atomics max diff %.3e\n", dt, Cc, L, pooled, sampling, rc, fwd_diff,
           fwd_same_as_plain, det_diff, worst);
    if (rc || fwd_diff || fwd_same_as_plain || det_diff || worst > 2e-5 || (dt == 0 && nonzero == 0)) ++bad;
    for (int k = 0; k < 2; ++k)
        for (int l = 0; l < L; ++l) { free(m[k][l]); free(mf[k][l]); free(g[k][l]); free(gf[k][l]); free(ga[k][l]); }
    free(boxes); free(img); free(flags); free(dout);
    return bad;
}

int main(int argc, char** argv) {
    int bad = 0;
    const int Cs[3] = {8, 24, 72};
    if (argc > 1 && !strcmp(argv[1], "mirror")) {                      // ./emu mirror: the mirrored entries alone
        const int cfg[4][4] = {{0, 4, 7, 2}, {3, 1, 7, 2}, {0, 4, 7, 0}, {0, 4, 2, 2}};
        for (int ci = 0; ci < 3; ++ci)
            for (int k = 0; k < 4; ++k) {
                if (ci == 2 && k > 0) continue;
                printf("mirror C %d cfg %d\n", Cs[ci], k);
                bad += run_mirror<float>(0, Cs[ci], cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3]);
                bad += run_mirror<_Float16>(1, Cs[ci], cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3]);
                bad += run_mirror<uint16_t>(2, Cs[ci], cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3]);
            }
        printf("bad %d\n", bad);
        return bad != 0;
    }
    const bool det_only = argc > 1 && !strcmp(argv[1], "det");       // ./emu det: the deterministic backward alone
    for (int ci = 0; ci < 3 && !det_only; ++ci) {
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
    for (int ci = 0; ci < 3; ++ci) {
        const int Cc = Cs[ci];
        const int cfg[4][4] = {{0, 4, 7, 2}, {3, 1, 7, 2}, {0, 4, 7, 0}, {0, 4, 2, 2}};
        for (int k = 0; k < 4; ++k) {
            printf("det C %d cfg %d\n", Cc, k);
            bad += run_det<float>(0, Cc, cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3], 12, 0);
            bad += run_det<_Float16>(1, Cc, cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3], 12, 0);
            bad += run_det<uint16_t>(2, Cc, cfg[k][0], cfg[k][1], cfg[k][2], cfg[k][3], 12, 0);
        }
    }
    bad += run_det<uint16_t>(2, 8, 0, 4, 7, 2, 0, 0);                  // no RoI: zeros everywhere
    bad += run_det<float>(0, 8, 0, 4, 7, 2, 12, 1);                    // the last RoI names image 7 of 3
    int64_t cnt[4]; skg_roi_align_layout_counts(cnt, 1);
    int64_t dc[2]; skg_roi_align_det_counts(dc, 1);
    printf("counts %lld %lld %lld %lld, det %lld %lld, bad %d\n", (long long)cnt[0], (long long)cnt[1], (long long)cnt[2], (long long)cnt[3],
           (long long)dc[0], (long long)dc[1], bad);
    return bad != 0;
}
