// skg_roialign.hip -- MultiScaleRoIAlign (the feature-cache producer in front of the interaction head).
//
// Reference call site: models/adamixer_transH_spatial_r50_models.py:158-162 (torchvision MultiScaleRoIAlign,
// featmap_names '0'..'3', output 7x7, sampling_ratio 2) used at heads/adamixer_transH_spatial_r50_head.py:387.
// torchvision is not in the image; the published algorithm is restated (oracle/roi_align_oracle.py is the CPU twin):
//   level  = clamp(floor(4 + log2(sqrt(area) / 224) + 1e-6), k_min, k_max) - k_min          (LevelMapper)
//   roi_align(aligned = False): roi scaled by the level's spatial scale, width/height clamped to >= 1, every output bin
//   averages sampling_ratio^2 bilinear samples; samples outside [-1, size] contribute 0.
// One thread per output element with the bin column fastest: neighbouring lanes read neighbouring feature pixels;
// the 16 taps of a bin hit L2.  HBM-bound on the [rois, C, 7, 7] write.
//
// Channels-last maps ([B, H_l, W_l, C] memory, what a channels_last backbone hands over) are read in place by the *_nhwc
// kernels further down: a workgroup owns one RoI x a slab of SKG_ROI_NHWC_SLAB (64) channels, a lane owns 16 bytes of
// consecutive channels (8 half / 4 fp32) of one bin, so every tap of a (bin, sample) is one contiguous row segment; the
// [slab][pooled^2] fp32 result tile is transposed through LDS and leaves as 16-byte stores (the backward stages d out the
// same way and issues its float atomics on consecutive addresses).  The arithmetic per output element is that of the NCHW
// kernels, operation for operation: only the tap addresses differ.
// Limits of the *_nhwc entries: C % 8 == 0 and pooled <= SKG_ROI_NHWC_MAX_POOLED (8: the 64 x (pooled^2 | 1) fp32 tile is
// static LDS, 16.25 KiB) else SKG_E_ARG; every level base, boxes, out / dout 16-byte aligned else SKG_E_ALIGN;
// n_rois * ceil(C / 64) workgroups <= 2^31 - 1 else SKG_E_LIMIT.
//
// Mirrored images (the *_mirror_* entries): image_mirror[b] != 0 makes every kernel address column W_l - 1 - x of image b
// wherever it addresses column x -- both x taps of every sample, on the RoI's level.  The coordinates, the outside test, the
// clamps, the weights and the order of the sums are untouched, so the result has the bits of running the plain kernel on a
// .flip(-1) copy of that image's maps.  MIR is a template parameter: the instances of a launch without flags contain no trace
// of it (their flag pointer, the last kernel argument, is never read).
#include <algorithm>
#include <atomic>
#include <type_traits>
#include "skg_common.h"

struct skg_roi_levels {
    const void* feat[SKG_ROI_MAX_LEVELS];     // [B, C, H_l, W_l] (map dtype of the launch; fp32 gradient maps backward)
    int H[SKG_ROI_MAX_LEVELS], W[SKG_ROI_MAX_LEVELS];
    float scale[SKG_ROI_MAX_LEVELS];
    int n_levels, k_min, k_max, C;
    float canonical_scale;
    int canonical_level;
};

// Element i of a map / output of dtype DT (SKG_DTYPE_*): loads widen exactly to fp32, stores round once (RNE).
template <int DT> struct skg_roi_elem;
template <> struct skg_roi_elem<SKG_DTYPE_F32> {
    typedef float T;
    static __device__ __forceinline__ float ld(const T* p, int64_t i) { return p[i]; }
    static __device__ __forceinline__ void st(T* p, int64_t i, float v) { p[i] = v; }
};
template <> struct skg_roi_elem<SKG_DTYPE_F16> {
    typedef _Float16 T;
    static __device__ __forceinline__ float ld(const T* p, int64_t i) { return (float)p[i]; }
    static __device__ __forceinline__ void st(T* p, int64_t i, float v) { p[i] = (_Float16)v; }
};
template <> struct skg_roi_elem<SKG_DTYPE_BF16> {
    typedef uint16_t T;                                             // bf16 bit patterns
    static __device__ __forceinline__ float ld(const T* p, int64_t i) { return __uint_as_float((uint32_t)p[i] << 16); }
    static __device__ __forceinline__ void st(T* p, int64_t i, float v) {
        const uint32_t u = __float_as_uint(v);                      // round to nearest even; nan -> the canonical quiet nan
        p[i] = v != v ? (uint16_t)0x7FC0 : (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
};

// Level and bin grid of one RoI: the one place that knows LevelMapper, the scaled corners, the >= 1 clamps and the grid.
struct skg_roi_geom {
    int l, H, W, gh, gw;
    float x1, y1, bw, bh, cnt;
};
__device__ __forceinline__ skg_roi_geom skg_roi_box_geom(const skg_roi_levels& L, const float4 b, int pooled, int sampling) {
    skg_roi_geom g;
    const float s = sqrtf((b.z - b.x) * (b.w - b.y));                  // LevelMapper (torchvision.ops.poolers.LevelMapper)
    float lv = floorf((float)L.canonical_level + log2f(s / L.canonical_scale) + 1e-6f);
    lv = fminf(fmaxf(lv, (float)L.k_min), (float)L.k_max);
    g.l = (int)lv - L.k_min;
    g.H = L.H[g.l]; g.W = L.W[g.l];
    const float sc = L.scale[g.l];
    const float x1 = b.x * sc, y1 = b.y * sc, x2 = b.z * sc, y2 = b.w * sc;
    const float rw = fmaxf(x2 - x1, 1.f), rh = fmaxf(y2 - y1, 1.f);
    g.x1 = x1; g.y1 = y1;
    g.bw = rw / (float)pooled; g.bh = rh / (float)pooled;
    g.gh = sampling > 0 ? sampling : (int)ceilf(rh / pooled);
    g.gw = sampling > 0 ? sampling : (int)ceilf(rw / pooled);
    g.cnt = fmaxf((float)(g.gh * g.gw), 1.f);
    return g;
}

// Coordinate of sample i of the n in bin `bin` along one axis.  Every kernel's bits depend on exactly this operation order:
// nothing is factored, reassociated or hoisted (size / n in particular).
__device__ __forceinline__ float skg_roi_coord(float origin, int bin, float size, int i, int n) {
    return origin + bin * size + (i + 0.5f) * size / (float)n;
}

// One axis of a sample, the one place that knows the outside test and the clamps: false when the sample lies outside on
// this axis, else the two taps and their weights l (high tap) / h (low tap).
struct skg_roi_axis {
    int low, high;
    float l, h;
};
__device__ __forceinline__ bool skg_roi_axis_sample(int size, float v, skg_roi_axis& a) {
    if (v < -1.0f || v > (float)size) return false;
    if (v <= 0.f) v = 0.f;
    int low = (int)v, high;
    if (low >= size - 1) { high = low = size - 1; v = (float)low; } else high = low + 1;
    a.low = low; a.high = high;
    a.l = v - low; a.h = 1.f - a.l;
    return true;
}

// The four taps of one sample and their weights; false: the sample lies outside and adds 0.
struct skg_roi_taps {
    int y_low, y_high, x_low, x_high;
    float w1, w2, w3, w4;
};
__device__ __forceinline__ bool skg_roi_sample(int H, int W, float y, float x, skg_roi_taps& t) {
    skg_roi_axis ay, ax;
    if (!skg_roi_axis_sample(H, y, ay) || !skg_roi_axis_sample(W, x, ax)) return false;
    t.y_low = ay.low; t.y_high = ay.high; t.x_low = ax.low; t.x_high = ax.high;
    t.w1 = ay.h * ax.h; t.w2 = ay.h * ax.l; t.w3 = ay.l * ax.h; t.w4 = ay.l * ax.l;
    return true;
}

// Tap columns of a mirrored image: the addresses only, after every coordinate, test, clamp and weight.
__device__ __forceinline__ void skg_roi_mirror_taps(int W, skg_roi_taps& t) {
    t.x_low = W - 1 - t.x_low; t.x_high = W - 1 - t.x_high;
}

// The [B, C, H, W] forward below keeps its own copy of the geometry, the coordinate and the sample rule (skg_bilinear): on
// skg_roi_box_geom / skg_roi_sample it computed the same bits but ran 0.4-0.5 us of 30-32 us slower on an MI355X (kernel-only
// times), with fewer instructions as with more.  Its expressions must stay those of the helpers above, operation
// for operation: tests/test_channels_last_roi_gpu.py and the host emulation compare its bits with the channels-last forward.
template <int DT, bool MIR>
__device__ __forceinline__ float skg_bilinear(const typename skg_roi_elem<DT>::T* __restrict__ f, int H, int W, float y,
                                              float x, bool mirror) {
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return 0.f;
    if (y <= 0.f) y = 0.f;
    if (x <= 0.f) x = 0.f;
    int y_low = (int)y, x_low = (int)x, y_high, x_high;
    if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
    if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
    const float ly = y - y_low, lx = x - x_low, hy = 1.f - ly, hx = 1.f - lx;
    if (MIR && mirror) { x_low = W - 1 - x_low; x_high = W - 1 - x_high; }         // the addresses only
    typedef skg_roi_elem<DT> E;
    const float v1 = E::ld(f, y_low * W + x_low), v2 = E::ld(f, y_low * W + x_high);
    const float v3 = E::ld(f, y_high * W + x_low), v4 = E::ld(f, y_high * W + x_high);
    return hy * hx * v1 + hy * lx * v2 + ly * hx * v3 + ly * lx * v4;
}

// MDT: map dtype, ODT: output dtype (SKG_DTYPE_*).  <F32, F32> is skg_roi_align_f32; the other instances only change
// how an element is loaded (widened exactly) and how the fp32 result is stored (rounded once).
template <int MDT, int ODT, bool MIR>
__global__ __launch_bounds__(256) void skg_roi_align_kernel(const skg_roi_levels L, const float* __restrict__ boxes,
                                                            const int32_t* __restrict__ box_image, int n_rois,
                                                            int pooled, int sampling,
                                                            typename skg_roi_elem<ODT>::T* __restrict__ out,
                                                            const int32_t* __restrict__ image_mirror) {
    typedef typename skg_roi_elem<MDT>::T TM;
    const int64_t total = (int64_t)n_rois * L.C * pooled * pooled;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int pw = (int)(idx % pooled);
        const int ph = (int)((idx / pooled) % pooled);
        const int c = (int)((idx / ((int64_t)pooled * pooled)) % L.C);
        const int n = (int)(idx / ((int64_t)pooled * pooled * L.C));
        const float4 b = *reinterpret_cast<const float4*>(boxes + 4 * (int64_t)n);
        // LevelMapper (torchvision.ops.poolers.LevelMapper)
        const float s = sqrtf((b.z - b.x) * (b.w - b.y));
        float lv = floorf((float)L.canonical_level + log2f(s / L.canonical_scale) + 1e-6f);
        lv = fminf(fmaxf(lv, (float)L.k_min), (float)L.k_max);
        const int l = (int)lv - L.k_min;
        const int H = L.H[l], W = L.W[l];
        const float sc = L.scale[l];
        const TM* f = static_cast<const TM*>(L.feat[l]) + ((int64_t)box_image[n] * L.C + c) * H * W;
        const float x1 = b.x * sc, y1 = b.y * sc, x2 = b.z * sc, y2 = b.w * sc;
        const float rw = fmaxf(x2 - x1, 1.f), rh = fmaxf(y2 - y1, 1.f);
        const float bw = rw / (float)pooled, bh = rh / (float)pooled;
        const int gh = sampling > 0 ? sampling : (int)ceilf(rh / pooled);
        const int gw = sampling > 0 ? sampling : (int)ceilf(rw / pooled);
        const float cnt = fmaxf((float)(gh * gw), 1.f);
        const bool mirror = MIR && image_mirror[box_image[n]] != 0;
        float acc = 0.f;
        for (int iy = 0; iy < gh; ++iy) {
            const float y = y1 + ph * bh + (iy + 0.5f) * bh / (float)gh;
            for (int ix = 0; ix < gw; ++ix) {
                const float x = x1 + pw * bw + (ix + 0.5f) * bw / (float)gw;
                acc += skg_bilinear<MDT, MIR>(f, H, W, y, x, mirror);
            }
        }
        skg_roi_elem<ODT>::st(out, idx, acc / cnt);
    }
}

// ------------------------------------------------------------------------------------------------ backward
// d feat[l][b, c, y, x] += sum over the samples that tapped it of  weight * d out[n, c, ph, pw] / count  (torchvision's
// roi_align backward: no gradient with respect to the boxes).  One thread per output element, float atomics on the
// feature gradients (zeroed by the caller): the summation order is not fixed, as in torchvision's kernel.
template <bool MIR>
__global__ __launch_bounds__(256) void skg_roi_align_bwd_kernel(const skg_roi_levels L, const float* __restrict__ boxes,
                                                                const int32_t* __restrict__ box_image, int n_rois,
                                                                int pooled, int sampling,
                                                                const float* __restrict__ dout,
                                                                const int32_t* __restrict__ image_mirror) {
    const int64_t total = (int64_t)n_rois * L.C * pooled * pooled;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int pw = (int)(idx % pooled);
        const int ph = (int)((idx / pooled) % pooled);
        const int c = (int)((idx / ((int64_t)pooled * pooled)) % L.C);
        const int n = (int)(idx / ((int64_t)pooled * pooled * L.C));
        const skg_roi_geom g = skg_roi_box_geom(L, *reinterpret_cast<const float4*>(boxes + 4 * (int64_t)n), pooled, sampling);
        const int W = g.W;
        float* f = static_cast<float*>(const_cast<void*>(L.feat[g.l])) + ((int64_t)box_image[n] * L.C + c) * g.H * W;   // gradient map of the level
        const float gr = dout[idx] / g.cnt;
        const bool mirror = MIR && image_mirror[box_image[n]] != 0;
        for (int iy = 0; iy < g.gh; ++iy) {
            const float y = skg_roi_coord(g.y1, ph, g.bh, iy, g.gh);
            for (int ix = 0; ix < g.gw; ++ix) {
                const float x = skg_roi_coord(g.x1, pw, g.bw, ix, g.gw);
                skg_roi_taps t;
                if (!skg_roi_sample(g.H, W, y, x, t)) continue;
                if (MIR && mirror) skg_roi_mirror_taps(W, t);
                atomicAdd(f + t.y_low * W + t.x_low, t.w1 * gr);
                atomicAdd(f + t.y_low * W + t.x_high, t.w2 * gr);
                atomicAdd(f + t.y_high * W + t.x_low, t.w3 * gr);
                atomicAdd(f + t.y_high * W + t.x_high, t.w4 * gr);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ channels-last maps
#define SKG_ROI_NHWC_SLAB 64
#define SKG_ROI_NHWC_MAX_POOLED 8
#define SKG_ROI_NHWC_TILE (SKG_ROI_NHWC_SLAB * (SKG_ROI_NHWC_MAX_POOLED * SKG_ROI_NHWC_MAX_POOLED + 1))

// 16 bytes of consecutive elements of dtype DT
template <int DT> union skg_roi_vec {
    uint4 q;
    typename skg_roi_elem<DT>::T e[16 / sizeof(typename skg_roi_elem<DT>::T)];
};

// grid = n_rois * n_slabs workgroups of 256: thread -> (bin group, 16-byte channel vector of the slab).
template <int MDT, int ODT, bool MIR>
__global__ __launch_bounds__(256) void skg_roi_align_nhwc_kernel(const skg_roi_levels L, const float* __restrict__ boxes,
                                                                 const int32_t* __restrict__ box_image, int n_slabs,
                                                                 int pooled, int sampling,
                                                                 typename skg_roi_elem<ODT>::T* __restrict__ out,
                                                                 const int32_t* __restrict__ image_mirror) {
    typedef skg_roi_elem<MDT> EM;
    typedef skg_roi_elem<ODT> EO;
    typedef typename EM::T TM;
    typedef typename EO::T TO;
    constexpr int VM = 16 / (int)sizeof(TM);                   // channels per lane
    constexpr int NV = SKG_ROI_NHWC_SLAB / VM;                 // lanes per bin
    constexpr int NG = 256 / NV;                               // bins in flight per workgroup
    constexpr int VO = 16 / (int)sizeof(TO);
    __shared__ float tile[SKG_ROI_NHWC_TILE];                  // [channel of the slab][pp | 1]
    const int n = (int)(blockIdx.x / (unsigned)n_slabs);
    const int c0 = (int)(blockIdx.x % (unsigned)n_slabs) * SKG_ROI_NHWC_SLAB;
    const int cs = min(SKG_ROI_NHWC_SLAB, L.C - c0);           // channels of this slab (a multiple of 8)
    const int pp = pooled * pooled, S = pp | 1;
    const skg_roi_geom g = skg_roi_box_geom(L, *reinterpret_cast<const float4*>(boxes + 4 * (int64_t)n), pooled, sampling);
    const int H = g.H, W = g.W;
    const int cl = ((int)threadIdx.x % NV) * VM;
    if (cl < cs) {
        const bool mirror = MIR && image_mirror[box_image[n]] != 0;
        const TM* f = static_cast<const TM*>(L.feat[g.l]) + (int64_t)box_image[n] * H * W * L.C + c0 + cl;
        for (int bin = (int)threadIdx.x / NV; bin < pp; bin += NG) {
            const int ph = bin / pooled, pw = bin - ph * pooled;
            float acc[VM];
#pragma unroll
            for (int j = 0; j < VM; ++j) acc[j] = 0.f;
            for (int iy = 0; iy < g.gh; ++iy) {
                const float y = skg_roi_coord(g.y1, ph, g.bh, iy, g.gh);
                for (int ix = 0; ix < g.gw; ++ix) {
                    const float x = skg_roi_coord(g.x1, pw, g.bw, ix, g.gw);
                    skg_roi_taps t;
                    if (!skg_roi_sample(H, W, y, x, t)) {
#pragma unroll
                        for (int j = 0; j < VM; ++j) acc[j] += 0.f;
                        continue;
                    }
                    if (MIR && mirror) skg_roi_mirror_taps(W, t);
                    skg_roi_vec<MDT> v1, v2, v3, v4;
                    v1.q = *reinterpret_cast<const uint4*>(f + ((int64_t)t.y_low * W + t.x_low) * L.C);
                    v2.q = *reinterpret_cast<const uint4*>(f + ((int64_t)t.y_low * W + t.x_high) * L.C);
                    v3.q = *reinterpret_cast<const uint4*>(f + ((int64_t)t.y_high * W + t.x_low) * L.C);
                    v4.q = *reinterpret_cast<const uint4*>(f + ((int64_t)t.y_high * W + t.x_high) * L.C);
#pragma unroll
                    for (int j = 0; j < VM; ++j)
                        acc[j] += t.w1 * EM::ld(v1.e, j) + t.w2 * EM::ld(v2.e, j) + t.w3 * EM::ld(v3.e, j) +
                                  t.w4 * EM::ld(v4.e, j);
                }
            }
#pragma unroll
            for (int j = 0; j < VM; ++j) tile[(cl + j) * S + bin] = acc[j] / g.cnt;
        }
    }
    __syncthreads();
    // the slab's cs * pp outputs are contiguous in [rois, C, pooled, pooled]: 16-byte stores
    TO* o = out + ((int64_t)n * L.C + c0) * pp;
    const int nvec = cs * pp / VO;
    for (int v = (int)threadIdx.x; v < nvec; v += 256) {
        skg_roi_vec<ODT> r;
#pragma unroll
        for (int j = 0; j < VO; ++j) {
            const int i = v * VO + j, c = i / pp;
            EO::st(r.e, j, tile[c * S + (i - c * pp)]);
        }
        *reinterpret_cast<uint4*>(o + (int64_t)v * VO) = r.q;
    }
}

// Backward into channels-last fp32 gradient maps: d out of the slab staged through LDS (16-byte loads); then a lane owns
// one channel and a wave one bin at a time (waves take the bins round-robin, the bin geometry is wave-uniform), so every
// atomic instruction of a full slab adds 256 contiguous bytes.  Same products as skg_roi_align_bwd_kernel.
template <bool MIR>
__global__ __launch_bounds__(256) void skg_roi_align_bwd_nhwc_kernel(const skg_roi_levels L, const float* __restrict__ boxes,
                                                                     const int32_t* __restrict__ box_image, int n_slabs,
                                                                     int pooled, int sampling,
                                                                     const float* __restrict__ dout,
                                                                     const int32_t* __restrict__ image_mirror) {
    constexpr int VM = 1, NV = SKG_ROI_NHWC_SLAB / VM, NG = 256 / NV;       // channels per lane, lanes per bin, bins in flight
    __shared__ float tile[SKG_ROI_NHWC_TILE];
    const int n = (int)(blockIdx.x / (unsigned)n_slabs);
    const int c0 = (int)(blockIdx.x % (unsigned)n_slabs) * SKG_ROI_NHWC_SLAB;
    const int cs = min(SKG_ROI_NHWC_SLAB, L.C - c0);
    const int pp = pooled * pooled, S = pp | 1;
    const float* d = dout + ((int64_t)n * L.C + c0) * pp;
    for (int v = (int)threadIdx.x; v < cs * pp / 4; v += 256) {
        const float4 q = *reinterpret_cast<const float4*>(d + (int64_t)v * 4);
        const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = v * 4 + j, c = i / pp;
            tile[c * S + (i - c * pp)] = e[j];
        }
    }
    __syncthreads();
    const skg_roi_geom g = skg_roi_box_geom(L, *reinterpret_cast<const float4*>(boxes + 4 * (int64_t)n), pooled, sampling);
    const int H = g.H, W = g.W;
    const int cl = ((int)threadIdx.x % NV) * VM;
    if (cl >= cs) return;
    const bool mirror = MIR && image_mirror[box_image[n]] != 0;
    float* f = static_cast<float*>(const_cast<void*>(L.feat[g.l])) + (int64_t)box_image[n] * H * W * L.C + c0 + cl;
    for (int bin = (int)threadIdx.x / NV; bin < pp; bin += NG) {
        const int ph = bin / pooled, pw = bin - ph * pooled;
        float gr[VM];
#pragma unroll
        for (int j = 0; j < VM; ++j) gr[j] = tile[(cl + j) * S + bin] / g.cnt;
        for (int iy = 0; iy < g.gh; ++iy) {
            const float y = skg_roi_coord(g.y1, ph, g.bh, iy, g.gh);
            for (int ix = 0; ix < g.gw; ++ix) {
                const float x = skg_roi_coord(g.x1, pw, g.bw, ix, g.gw);
                skg_roi_taps t;
                if (!skg_roi_sample(H, W, y, x, t)) continue;
                if (MIR && mirror) skg_roi_mirror_taps(W, t);
                float* p1 = f + ((int64_t)t.y_low * W + t.x_low) * L.C;
                float* p2 = f + ((int64_t)t.y_low * W + t.x_high) * L.C;
                float* p3 = f + ((int64_t)t.y_high * W + t.x_low) * L.C;
                float* p4 = f + ((int64_t)t.y_high * W + t.x_high) * L.C;
#pragma unroll
                for (int j = 0; j < VM; ++j) atomicAdd(p1 + j, t.w1 * gr[j]);
#pragma unroll
                for (int j = 0; j < VM; ++j) atomicAdd(p2 + j, t.w2 * gr[j]);
#pragma unroll
                for (int j = 0; j < VM; ++j) atomicAdd(p3 + j, t.w3 * gr[j]);
#pragma unroll
                for (int j = 0; j < VM; ++j) atomicAdd(p4 + j, t.w4 * gr[j]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ deterministic backward
// Owner-computes gather, no atomics: one workgroup per (level, image, pixel tile, channel slab), all levels in one launch.
// Every gradient element (l, b, c, y, x) is produced by exactly one thread and stored exactly once -- also the elements no
// RoI touches (0) and the images without boxes -- so the maps need no zero fill and hold the maps' dtype directly.
// The sum of an element, in this fixed order whatever the layout, tile, slab or grid:
//     acc = 0.f; RoIs in ascending index; within a RoI the sample rows sy = ph * gh + iy ascending, then the sample columns
//     sx = pw * gw + ix ascending; within a sample its taps in the order 1..4 of skg_roi_taps; a tap counts when its
//     coordinates equal (y, x) (a clamped sample can hit one pixel with two taps); term = (wy * wx) * (dout[r, c, ph, pw] / cnt),
//     the product t.wK * gr of the atomics kernels; fp32 accumulation, one store through skg_roi_elem<DT>::st.
// A workgroup's threads each take a RoI of a chunk of SKG_ROI_DET_CHUNK, recompute its geometry (skg_roi_box_geom: the
// forward's level bit for bit), test a superset of its tap rectangle against the tile and compact the hits in ascending RoI
// index into an LDS list; the chunks follow each other, so n_rois is unbounded and no workspace is needed.  The per-pixel
// tap tests walk the 1-D sample rows and columns with the forward's expressions (skg_roi_sample's rules per axis): the
// sampling is never inverted analytically, and the walk indexes no memory by a tap coordinate.
// A workgroup belongs to one image, so its mirror flag is uniform: the thread that owns physical pixel (py, px) of a mirrored
// image runs the walk for the virtual pixel (py, W - 1 - px), the tile's rectangle is listed as [W - 1 - tx1, W - 1 - tx0], and
// the store goes to the physical pixel.  The order above holds in the virtual frame: the bits of autograd through .flip(-1).
#define SKG_ROI_DET_CHUNK 256
#define SKG_ROI_DET_TW 32                      // [B, C, H, W]: 32 x 8 pixels, lanes along x, 16 channels per slab
#define SKG_ROI_DET_TH 8
#define SKG_ROI_DET_CS 16
#define SKG_ROI_DET_NT 8                       // channels-last: 8 x 8 pixels, lanes along channels, SKG_ROI_NHWC_SLAB channels

struct skg_roi_det_grid {
    int tiles_x[SKG_ROI_MAX_LEVELS], tiles_y[SKG_ROI_MAX_LEVELS];
    unsigned start[SKG_ROI_MAX_LEVELS + 1];    // first workgroup of a level; per level: image slowest, tile, slab fastest
    int n_slabs;
};

// a listed RoI: what the tap walk needs of skg_roi_geom
struct skg_roi_det_item {
    int r, gh, gw;
    float x1, y1, bw, bh, cnt;
};

// The taps of RoI `it` that land on pixel (py, px), in the contract's order: add(bin, wy * wx) per tap.
template <class F>
__device__ __forceinline__ void skg_roi_det_walk(const skg_roi_det_item& it, int H, int W, int pooled, int py, int px, F add) {
    for (int ph = 0; ph < pooled; ++ph)
        for (int iy = 0; iy < it.gh; ++iy) {
            const float y = skg_roi_coord(it.y1, ph, it.bh, iy, it.gh);
            skg_roi_axis ay;
            if (!skg_roi_axis_sample(H, y, ay)) continue;
            const bool yl = ay.low == py, yh = ay.high == py;
            if (!yl && !yh) continue;
            for (int pw = 0; pw < pooled; ++pw)
                for (int ix = 0; ix < it.gw; ++ix) {
                    const float x = skg_roi_coord(it.x1, pw, it.bw, ix, it.gw);
                    skg_roi_axis ax;
                    if (!skg_roi_axis_sample(W, x, ax)) continue;
                    const bool xl = ax.low == px, xh = ax.high == px;
                    if (!xl && !xh) continue;
#pragma unroll 1
                    for (int k = 0; k < 4; ++k) {                      // taps 1..4: (low, low) (low, high) (high, low) (high, high)
                        if (!((k < 2 ? yl : yh) && ((k & 1) ? xh : xl))) continue;
                        add(ph * pooled + pw, (k < 2 ? ay.h : ay.l) * ((k & 1) ? ax.l : ax.h));
                    }
                }
        }
}

// RoIs chunk0 .. chunk0 + 255 of image b on level l whose taps can reach the tile [ty0, ty1] x [tx0, tx1]: compacted in
// ascending index into s_item, their number in *s_n (valid after the call, which ends in a barrier).  The rectangle test is
// a superset (first / last sample of each axis, a pixel of margin for the rounding of the coordinates): a listed RoI without
// a tap on a pixel adds nothing there.  Compared in float, so no box value is converted to an integer.
__device__ __forceinline__ int skg_roi_det_list(const skg_roi_levels& L, const float* __restrict__ boxes,
                                                const int32_t* __restrict__ box_image, int n_rois, int chunk0, int l, int b,
                                                int ty0, int ty1, int tx0, int tx1, int pooled, int sampling,
                                                uint32_t* s_hit, skg_roi_det_item* s_item, int* s_n) {
    const int tid = (int)threadIdx.x, r = chunk0 + tid;
    unsigned char* hb = reinterpret_cast<unsigned char*>(s_hit);
    bool hit = false;
    skg_roi_det_item it;
    if (r < n_rois && box_image[r] == b) {
        const skg_roi_geom g = skg_roi_box_geom(L, *reinterpret_cast<const float4*>(boxes + 4 * (int64_t)r), pooled, sampling);
        if (g.l == l) {
            const float yf = skg_roi_coord(g.y1, 0, g.bh, 0, g.gh), ye = skg_roi_coord(g.y1, pooled - 1, g.bh, g.gh - 1, g.gh);
            const float xf = skg_roi_coord(g.x1, 0, g.bw, 0, g.gw), xe = skg_roi_coord(g.x1, pooled - 1, g.bw, g.gw - 1, g.gw);
            hit = !(floorf(fmaxf(ye, 0.f)) + 2.f < (float)ty0) && !(floorf(fmaxf(yf, 0.f)) - 1.f > (float)ty1) &&
                  !(floorf(fmaxf(xe, 0.f)) + 2.f < (float)tx0) && !(floorf(fmaxf(xf, 0.f)) - 1.f > (float)tx1);
            it.r = r; it.gh = g.gh; it.gw = g.gw;
            it.x1 = g.x1; it.y1 = g.y1; it.bw = g.bw; it.bh = g.bh; it.cnt = g.cnt;
        }
    }
    hb[tid] = hit ? 1 : 0;
    __syncthreads();
    int pos = 0;                                                       // hits of the threads below this one
    for (int w = 0; w < tid / 4; ++w) pos += (int)((s_hit[w] * 0x01010101u) >> 24);
    for (int k = tid & ~3; k < tid; ++k) pos += hb[k];
    if (hit) s_item[pos] = it;
    if (tid == SKG_ROI_DET_CHUNK - 1) *s_n = pos + (hit ? 1 : 0);
    __syncthreads();
    return *s_n;
}

// workgroup -> (level, image, tile, slab)
__device__ __forceinline__ void skg_roi_det_item_of_block(const skg_roi_levels& L, const skg_roi_det_grid& G, int& l, int& b,
                                                          int& tile_y, int& tile_x, int& slab) {
    l = 0;
    while (l + 1 < L.n_levels && blockIdx.x >= G.start[l + 1]) ++l;
    unsigned rem = blockIdx.x - G.start[l];
    slab = (int)(rem % (unsigned)G.n_slabs); rem /= (unsigned)G.n_slabs;
    const unsigned nt = (unsigned)(G.tiles_x[l] * G.tiles_y[l]);
    const unsigned t = rem % nt;
    b = (int)(rem / nt);
    tile_y = (int)(t / (unsigned)G.tiles_x[l]); tile_x = (int)(t % (unsigned)G.tiles_x[l]);
}

// [B, C, H, W] gradient maps of dtype DT: a thread owns one pixel of the 32 x 8 tile (lanes along x) and the slab's channels.
template <int DT, bool MIR>
__global__ __launch_bounds__(256) void skg_roi_align_bwd_det_kernel(const skg_roi_levels L, const skg_roi_det_grid G,
                                                                    const float* __restrict__ boxes,
                                                                    const int32_t* __restrict__ box_image, int n_rois,
                                                                    int pooled, int sampling, const float* __restrict__ dout,
                                                                    const int32_t* __restrict__ image_mirror) {
    typedef skg_roi_elem<DT> E;
    typedef typename E::T T;
    constexpr int CS = SKG_ROI_DET_CS;
    __shared__ uint32_t s_hit[SKG_ROI_DET_CHUNK / 4];
    __shared__ skg_roi_det_item s_item[SKG_ROI_DET_CHUNK];
    __shared__ int s_n;
    int l, b, tile_y, tile_x, slab;
    skg_roi_det_item_of_block(L, G, l, b, tile_y, tile_x, slab);
    const int H = L.H[l], W = L.W[l];
    const int ty0 = tile_y * SKG_ROI_DET_TH, tx0 = tile_x * SKG_ROI_DET_TW;
    const int ty1 = min(ty0 + SKG_ROI_DET_TH, H) - 1, tx1 = min(tx0 + SKG_ROI_DET_TW, W) - 1;
    const int py = ty0 + (int)threadIdx.x / SKG_ROI_DET_TW, px = tx0 + (int)threadIdx.x % SKG_ROI_DET_TW;
    const bool own = py < H && px < W;
    const bool mirror = MIR && image_mirror[b] != 0;
    const int vx = mirror ? W - 1 - px : px;                           // the pixel of the walk (virtual frame)
    const int lx0 = mirror ? W - 1 - tx1 : tx0, lx1 = mirror ? W - 1 - tx0 : tx1;
    const int c0 = slab * CS, cs = min(CS, L.C - c0), pp = pooled * pooled;
    float acc[CS];
#pragma unroll
    for (int j = 0; j < CS; ++j) acc[j] = 0.f;
    for (int chunk0 = 0; chunk0 < n_rois; chunk0 += SKG_ROI_DET_CHUNK) {
        const int n = skg_roi_det_list(L, boxes, box_image, n_rois, chunk0, l, b, ty0, ty1, lx0, lx1, pooled, sampling, s_hit,
                                       s_item, &s_n);
        if (!own) continue;
        for (int i = 0; i < n; ++i) {
            const skg_roi_det_item it = s_item[i];
            const float* d = dout + ((int64_t)it.r * L.C + c0) * pp;
            skg_roi_det_walk(it, H, W, pooled, py, vx, [&](int bin, float w) {
#pragma unroll
                for (int j = 0; j < CS; ++j)
                    if (j < cs) acc[j] += w * (d[(int64_t)j * pp + bin] / it.cnt);
            });
        }
    }
    if (!own) return;
    T* f = static_cast<T*>(const_cast<void*>(L.feat[l])) + ((int64_t)b * L.C + c0) * H * W + (int64_t)py * W + px;
#pragma unroll
    for (int j = 0; j < CS; ++j)
        if (j < cs) E::st(f, (int64_t)j * H * W, acc[j]);
}

// Channels-last gradient maps of dtype DT: a lane owns 16 bytes of consecutive channels (4 fp32 / 8 half) of the slab for
// 64 / NG pixels of the 8 x 8 tile; d out of a listed RoI's slab is staged through LDS with 16-byte loads (divided by the
// sample count on the way: the gr of the atomics kernel) and the gradient leaves as 16-byte stores.
template <int DT, bool MIR>
__global__ __launch_bounds__(256) void skg_roi_align_bwd_det_nhwc_kernel(const skg_roi_levels L, const skg_roi_det_grid G,
                                                                         const float* __restrict__ boxes,
                                                                         const int32_t* __restrict__ box_image, int n_rois,
                                                                         int pooled, int sampling,
                                                                         const float* __restrict__ dout,
                                                                         const int32_t* __restrict__ image_mirror) {
    typedef skg_roi_elem<DT> E;
    typedef typename E::T T;
    constexpr int VG = 16 / (int)sizeof(T);                    // channels per lane
    constexpr int NV = SKG_ROI_NHWC_SLAB / VG;                 // lanes per pixel
    constexpr int NG = 256 / NV;                               // pixels in flight
    constexpr int NP = SKG_ROI_DET_NT * SKG_ROI_DET_NT / NG;   // pixels per thread
    __shared__ float tile[SKG_ROI_NHWC_TILE];                  // [channel of the slab][pp | 1] of d out / cnt
    __shared__ uint32_t s_hit[SKG_ROI_DET_CHUNK / 4];
    __shared__ skg_roi_det_item s_item[SKG_ROI_DET_CHUNK];
    __shared__ int s_n;
    int l, b, tile_y, tile_x, slab;
    skg_roi_det_item_of_block(L, G, l, b, tile_y, tile_x, slab);
    const int H = L.H[l], W = L.W[l];
    const int ty0 = tile_y * SKG_ROI_DET_NT, tx0 = tile_x * SKG_ROI_DET_NT;
    const int ty1 = min(ty0 + SKG_ROI_DET_NT, H) - 1, tx1 = min(tx0 + SKG_ROI_DET_NT, W) - 1;
    const int c0 = slab * SKG_ROI_NHWC_SLAB, cs = min(SKG_ROI_NHWC_SLAB, L.C - c0);    // cs: a multiple of 8
    const int pp = pooled * pooled, S = pp | 1;
    const int cl = ((int)threadIdx.x % NV) * VG, grp = (int)threadIdx.x / NV;
    const bool mirror = MIR && image_mirror[b] != 0;
    const int lx0 = mirror ? W - 1 - tx1 : tx0, lx1 = mirror ? W - 1 - tx0 : tx1;
    int py[NP], px[NP];
    bool own[NP];
    float acc[NP][VG];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = grp + k * NG;
        py[k] = ty0 + p / SKG_ROI_DET_NT; px[k] = tx0 + p % SKG_ROI_DET_NT;
        own[k] = cl < cs && py[k] < H && px[k] < W;
#pragma unroll
        for (int j = 0; j < VG; ++j) acc[k][j] = 0.f;
    }
    for (int chunk0 = 0; chunk0 < n_rois; chunk0 += SKG_ROI_DET_CHUNK) {
        const int n = skg_roi_det_list(L, boxes, box_image, n_rois, chunk0, l, b, ty0, ty1, lx0, lx1, pooled, sampling, s_hit,
                                       s_item, &s_n);
        for (int i = 0; i < n; ++i) {
            const skg_roi_det_item it = s_item[i];
            const float* d = dout + ((int64_t)it.r * L.C + c0) * pp;
            for (int v = (int)threadIdx.x; v < cs * pp / 4; v += 256) {
                const float4 q = *reinterpret_cast<const float4*>(d + (int64_t)v * 4);
                const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int t = v * 4 + j, c = t / pp;
                    tile[c * S + (t - c * pp)] = e[j] / it.cnt;
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                if (!own[k]) continue;
                skg_roi_det_walk(it, H, W, pooled, py[k], mirror ? W - 1 - px[k] : px[k], [&](int bin, float w) {
#pragma unroll
                    for (int j = 0; j < VG; ++j) acc[k][j] += w * tile[(cl + j) * S + bin];
                });
            }
            __syncthreads();
        }
    }
    T* f = static_cast<T*>(const_cast<void*>(L.feat[l])) + (int64_t)b * H * W * L.C + c0 + cl;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (!own[k]) continue;
        skg_roi_vec<DT> r;
#pragma unroll
        for (int j = 0; j < VG; ++j) E::st(r.e, j, acc[k][j]);
        *reinterpret_cast<uint4*>(f + ((int64_t)py[k] * W + px[k]) * L.C) = r.q;
    }
}

// ------------------------------------------------------------------------------------------------ entries
// launches since the last reset: forward NCHW, forward NHWC, backward NCHW, backward NHWC (skg_roi_align_layout_counts)
static std::atomic<long long> g_roi_layout_counts[4];

extern "C" void skg_roi_align_layout_counts(int64_t* out4, int reset) {
    for (int i = 0; i < 4; ++i) {
        if (out4) out4[i] = g_roi_layout_counts[i].load(std::memory_order_relaxed);
        if (reset) g_roi_layout_counts[i].store(0, std::memory_order_relaxed);
    }
}

static int skg_roi_levels_fill(skg_roi_levels& L, const void* const* feats_host, const int32_t* H_host,
                               const int32_t* W_host, const float* scales_host, int n_levels, int C, int k_min, int k_max,
                               float canonical_scale, int canonical_level) {
    for (int l = 0; l < SKG_ROI_MAX_LEVELS; ++l) {
        const bool in = l < n_levels;
        L.feat[l] = in ? feats_host[l] : nullptr;
        L.H[l] = in ? H_host[l] : 0; L.W[l] = in ? W_host[l] : 0; L.scale[l] = in ? scales_host[l] : 0.f;
        if (in && (!L.feat[l] || L.H[l] <= 0 || L.W[l] <= 0)) return SKG_E_ARG;
    }
    L.n_levels = n_levels; L.k_min = k_min; L.k_max = k_max; L.C = C;
    L.canonical_scale = canonical_scale; L.canonical_level = canonical_level;
    return 0;
}

// The argument check of every launching entry, in the order that decides which code wins; fills L.
//   nhwc: the channels-last limits -- C % 8 and pooled <= SKG_ROI_NHWC_MAX_POOLED, `io` (out / dout) and every level base
//         16-byte aligned;
//   det:  a deterministic entry -- n_images is checked, and without a RoI it still launches (the maps are written), where
//         the others have nothing to do; the level bases are left to its grid loop, which reports them level by level
//         between the workgroup counts.
//   dt0, dt1: the entry's dtype codes (an entry with one passes it twice, an fp32-only entry SKG_DTYPE_F32).
//   image_mirror: the per-image mirror flags (device, n_images of them) or null; with flags n_images is checked too.
// Returns SKG_E_* or 0; *nothing: 0 was returned because there is no RoI and the entry is not deterministic (no launch).
static int skg_roi_check(bool nhwc, bool det, skg_roi_levels& L, const void* const* feats_host, int dt0, int dt1,
                         const int32_t* H_host, const int32_t* W_host, const float* scales_host, int n_levels, int C, int k_min,
                         int k_max, float canonical_scale, int canonical_level, const float* boxes, const int32_t* box_image,
                         int n_rois, int n_images, int pooled, const void* io, const int32_t* image_mirror, bool* nothing) {
    *nothing = false;
    if (n_levels < 1 || n_levels > SKG_ROI_MAX_LEVELS || C <= 0 || pooled <= 0 || n_rois < 0 || k_max - k_min + 1 != n_levels)
        return SKG_E_ARG;
    if (dt0 < SKG_DTYPE_F32 || dt0 > SKG_DTYPE_BF16 || dt1 < SKG_DTYPE_F32 || dt1 > SKG_DTYPE_BF16) return SKG_E_ARG;
    if ((det || image_mirror) && n_images <= 0) return SKG_E_ARG;
    if (nhwc && ((C & 7) || pooled > SKG_ROI_NHWC_MAX_POOLED)) return SKG_E_ARG;     // 16-byte channel vectors; the LDS tile
    if (n_rois == 0 && !det) { *nothing = true; return 0; }
    if (!feats_host || !H_host || !W_host || !scales_host) return SKG_E_ARG;
    if (n_rois > 0 && (!boxes || !box_image || !io)) return SKG_E_ARG;
    if (n_rois > 0 && (!skg_aligned16(boxes) || (nhwc && !skg_aligned16(io)))) return SKG_E_ALIGN;
    const int rc = skg_roi_levels_fill(L, feats_host, H_host, W_host, scales_host, n_levels, C, k_min, k_max, canonical_scale,
                                       canonical_level);
    if (rc) return rc;
    for (int l = 0; nhwc && !det && l < n_levels; ++l)
        if (!skg_aligned16(L.feat[l])) return SKG_E_ALIGN;
    return 0;
}

// f(std::integral_constant<int, dt>()) for a checked dtype code: the template argument of a kernel from a run-time value
template <class F>
static void skg_roi_with_dtype(int dt, F f) {
    switch (dt) {
        case SKG_DTYPE_F32: f(std::integral_constant<int, SKG_DTYPE_F32>()); break;
        case SKG_DTYPE_F16: f(std::integral_constant<int, SKG_DTYPE_F16>()); break;
        default: f(std::integral_constant<int, SKG_DTYPE_BF16>()); break;
    }
}

// f(std::true_type / std::false_type): the MIR argument of a kernel -- flags given or not
template <class F>
static void skg_roi_with_mirror(const int32_t* image_mirror, F f) {
    if (image_mirror) f(std::true_type()); else f(std::false_type());
}

// The four *_mirror_* entries below: every check, the counter, one launch.  The entries without flags forward to them
// with a null pointer and launch the instances they always launched.

// [B, C, H, W] kernels: one thread per output element, grid-stride beyond 256 * 64 workgroups
static dim3 skg_roi_nchw_grid(int n_rois, int C, int pooled) {
    return dim3((unsigned)std::min<int64_t>(((int64_t)n_rois * C * pooled * pooled + 255) / 256, 256 * 64));
}

extern "C" int skg_roi_align_mirror_x(const void* const* feats_host, int map_dtype, const int32_t* H_host,
                                      const int32_t* W_host, const float* scales_host, int n_levels, int C, int k_min,
                                      int k_max, float canonical_scale, int canonical_level, const float* boxes,
                                      const int32_t* box_image, int n_rois, int pooled, int sampling, void* out,
                                      int out_dtype, const int32_t* image_mirror, int n_images, void* stream) {
    skg_roi_levels L;
    bool nothing;
    const int rc = skg_roi_check(false, false, L, feats_host, map_dtype, out_dtype, H_host, W_host, scales_host, n_levels, C,
                                 k_min, k_max, canonical_scale, canonical_level, boxes, box_image, n_rois, n_images, pooled, out,
                                 image_mirror, &nothing);
    if (rc || nothing) return rc;
    g_roi_layout_counts[0].fetch_add(1, std::memory_order_relaxed);
    skg_roi_with_dtype(map_dtype, [&](auto m) {
        skg_roi_with_dtype(out_dtype, [&](auto o) {
            skg_roi_with_mirror(image_mirror, [&](auto mir) {
                hipLaunchKernelGGL((skg_roi_align_kernel<decltype(m)::value, decltype(o)::value, decltype(mir)::value>),
                                   skg_roi_nchw_grid(n_rois, C, pooled), dim3(256), 0, (hipStream_t)stream, L, boxes, box_image,
                                   n_rois, pooled, sampling, static_cast<typename skg_roi_elem<decltype(o)::value>::T*>(out),
                                   image_mirror);
            });
        });
    });
    return skg_launch_status();
}

extern "C" int skg_roi_align_x(const void* const* feats_host, int map_dtype, const int32_t* H_host,
                               const int32_t* W_host, const float* scales_host, int n_levels, int C, int k_min,
                               int k_max, float canonical_scale, int canonical_level, const float* boxes,
                               const int32_t* box_image, int n_rois, int pooled, int sampling, void* out, int out_dtype,
                               void* stream) {
    return skg_roi_align_mirror_x(feats_host, map_dtype, H_host, W_host, scales_host, n_levels, C, k_min, k_max,
                                  canonical_scale, canonical_level, boxes, box_image, n_rois, pooled, sampling, out, out_dtype,
                                  nullptr, 0, stream);
}

extern "C" int skg_roi_align_f32(const float* const* feats_host, const int32_t* H_host, const int32_t* W_host,
                                 const float* scales_host, int n_levels, int C, int k_min, int k_max,
                                 float canonical_scale, int canonical_level, const float* boxes,
                                 const int32_t* box_image, int n_rois, int pooled, int sampling, float* out,
                                 void* stream) {
    return skg_roi_align_x(reinterpret_cast<const void* const*>(feats_host), SKG_DTYPE_F32, H_host, W_host, scales_host,
                           n_levels, C, k_min, k_max, canonical_scale, canonical_level, boxes, box_image, n_rois,
                           pooled, sampling, out, SKG_DTYPE_F32, stream);
}

extern "C" int skg_roi_align_bwd_mirror_f32(float* const* dfeats_host, const int32_t* H_host, const int32_t* W_host,
                                            const float* scales_host, int n_levels, int C, int k_min, int k_max,
                                            float canonical_scale, int canonical_level, const float* boxes,
                                            const int32_t* box_image, int n_rois, int pooled, int sampling,
                                            const float* dout, const int32_t* image_mirror, int n_images, void* stream) {
    skg_roi_levels L;
    bool nothing;
    const int rc = skg_roi_check(false, false, L, reinterpret_cast<const void* const*>(dfeats_host), SKG_DTYPE_F32,
                                 SKG_DTYPE_F32, H_host, W_host, scales_host, n_levels, C, k_min, k_max, canonical_scale,
                                 canonical_level, boxes, box_image, n_rois, n_images, pooled, dout, image_mirror, &nothing);
    if (rc || nothing) return rc;
    g_roi_layout_counts[2].fetch_add(1, std::memory_order_relaxed);
    skg_roi_with_mirror(image_mirror, [&](auto mir) {
        hipLaunchKernelGGL(skg_roi_align_bwd_kernel<decltype(mir)::value>, skg_roi_nchw_grid(n_rois, C, pooled), dim3(256), 0,
                           (hipStream_t)stream, L, boxes, box_image, n_rois, pooled, sampling, dout, image_mirror);
    });
    return skg_launch_status();
}

extern "C" int skg_roi_align_bwd_f32(float* const* dfeats_host, const int32_t* H_host, const int32_t* W_host,
                                     const float* scales_host, int n_levels, int C, int k_min, int k_max,
                                     float canonical_scale, int canonical_level, const float* boxes,
                                     const int32_t* box_image, int n_rois, int pooled, int sampling, const float* dout,
                                     void* stream) {
    return skg_roi_align_bwd_mirror_f32(dfeats_host, H_host, W_host, scales_host, n_levels, C, k_min, k_max, canonical_scale,
                                        canonical_level, boxes, box_image, n_rois, pooled, sampling, dout, nullptr, 0, stream);
}

// channels-last: one workgroup per (RoI, slab of SKG_ROI_NHWC_SLAB channels)
extern "C" int skg_roi_align_mirror_nhwc_x(const void* const* feats_host, int map_dtype, const int32_t* H_host,
                                           const int32_t* W_host, const float* scales_host, int n_levels, int C, int k_min,
                                           int k_max, float canonical_scale, int canonical_level, const float* boxes,
                                           const int32_t* box_image, int n_rois, int pooled, int sampling, void* out,
                                           int out_dtype, const int32_t* image_mirror, int n_images, void* stream) {
    skg_roi_levels L;
    bool nothing;
    const int rc = skg_roi_check(true, false, L, feats_host, map_dtype, out_dtype, H_host, W_host, scales_host, n_levels, C,
                                 k_min, k_max, canonical_scale, canonical_level, boxes, box_image, n_rois, n_images, pooled, out,
                                 image_mirror, &nothing);
    if (rc || nothing) return rc;
    const int n_slabs = (C + SKG_ROI_NHWC_SLAB - 1) / SKG_ROI_NHWC_SLAB;
    if ((int64_t)n_rois * n_slabs > 0x7fffffffLL) return SKG_E_LIMIT;
    g_roi_layout_counts[1].fetch_add(1, std::memory_order_relaxed);
    skg_roi_with_dtype(map_dtype, [&](auto m) {
        skg_roi_with_dtype(out_dtype, [&](auto o) {
            skg_roi_with_mirror(image_mirror, [&](auto mir) {
                hipLaunchKernelGGL((skg_roi_align_nhwc_kernel<decltype(m)::value, decltype(o)::value, decltype(mir)::value>),
                                   dim3((unsigned)(n_rois * n_slabs)), dim3(256), 0, (hipStream_t)stream, L, boxes, box_image,
                                   n_slabs, pooled, sampling, static_cast<typename skg_roi_elem<decltype(o)::value>::T*>(out),
                                   image_mirror);
            });
        });
    });
    return skg_launch_status();
}

extern "C" int skg_roi_align_nhwc_x(const void* const* feats_host, int map_dtype, const int32_t* H_host,
                                    const int32_t* W_host, const float* scales_host, int n_levels, int C, int k_min,
                                    int k_max, float canonical_scale, int canonical_level, const float* boxes,
                                    const int32_t* box_image, int n_rois, int pooled, int sampling, void* out,
                                    int out_dtype, void* stream) {
    return skg_roi_align_mirror_nhwc_x(feats_host, map_dtype, H_host, W_host, scales_host, n_levels, C, k_min, k_max,
                                       canonical_scale, canonical_level, boxes, box_image, n_rois, pooled, sampling, out,
                                       out_dtype, nullptr, 0, stream);
}

extern "C" int skg_roi_align_bwd_mirror_nhwc_f32(float* const* dfeats_host, const int32_t* H_host, const int32_t* W_host,
                                                 const float* scales_host, int n_levels, int C, int k_min, int k_max,
                                                 float canonical_scale, int canonical_level, const float* boxes,
                                                 const int32_t* box_image, int n_rois, int pooled, int sampling,
                                                 const float* dout, const int32_t* image_mirror, int n_images,
                                                 void* stream) {
    skg_roi_levels L;
    bool nothing;
    const int rc = skg_roi_check(true, false, L, reinterpret_cast<const void* const*>(dfeats_host), SKG_DTYPE_F32,
                                 SKG_DTYPE_F32, H_host, W_host, scales_host, n_levels, C, k_min, k_max, canonical_scale,
                                 canonical_level, boxes, box_image, n_rois, n_images, pooled, dout, image_mirror, &nothing);
    if (rc || nothing) return rc;
    const int n_slabs = (C + SKG_ROI_NHWC_SLAB - 1) / SKG_ROI_NHWC_SLAB;
    if ((int64_t)n_rois * n_slabs > 0x7fffffffLL) return SKG_E_LIMIT;
    g_roi_layout_counts[3].fetch_add(1, std::memory_order_relaxed);
    skg_roi_with_mirror(image_mirror, [&](auto mir) {
        hipLaunchKernelGGL(skg_roi_align_bwd_nhwc_kernel<decltype(mir)::value>, dim3((unsigned)(n_rois * n_slabs)), dim3(256), 0,
                           (hipStream_t)stream, L, boxes, box_image, n_slabs, pooled, sampling, dout, image_mirror);
    });
    return skg_launch_status();
}

extern "C" int skg_roi_align_bwd_nhwc_f32(float* const* dfeats_host, const int32_t* H_host, const int32_t* W_host,
                                          const float* scales_host, int n_levels, int C, int k_min, int k_max,
                                          float canonical_scale, int canonical_level, const float* boxes,
                                          const int32_t* box_image, int n_rois, int pooled, int sampling,
                                          const float* dout, void* stream) {
    return skg_roi_align_bwd_mirror_nhwc_f32(dfeats_host, H_host, W_host, scales_host, n_levels, C, k_min, k_max,
                                             canonical_scale, canonical_level, boxes, box_image, n_rois, pooled, sampling, dout,
                                             nullptr, 0, stream);
}

// deterministic backward launches since the last reset: [B, C, H, W], channels-last (skg_roi_align_det_counts)
static std::atomic<long long> g_roi_det_counts[2];

extern "C" void skg_roi_align_det_counts(int64_t* out2, int reset) {
    for (int i = 0; i < 2; ++i) {
        if (out2) out2[i] = g_roi_det_counts[i].load(std::memory_order_relaxed);
        if (reset) g_roi_det_counts[i].store(0, std::memory_order_relaxed);
    }
}

// all four deterministic entries: every check, then one launch
static int skg_roi_align_bwd_det(bool nhwc, void* const* dfeats_host, int grad_dtype, const int32_t* H_host,
                                 const int32_t* W_host, const float* scales_host, int n_levels, int C, int k_min, int k_max,
                                 float canonical_scale, int canonical_level, const float* boxes, const int32_t* box_image,
                                 int n_rois, int n_images, int pooled, int sampling, const float* dout,
                                 const int32_t* image_mirror, void* stream) {
    skg_roi_levels L;
    bool nothing;
    const int rc = skg_roi_check(nhwc, true, L, reinterpret_cast<const void* const*>(dfeats_host), grad_dtype, grad_dtype,
                                 H_host, W_host, scales_host, n_levels, C, k_min, k_max, canonical_scale, canonical_level, boxes,
                                 box_image, n_rois, n_images, pooled, dout, image_mirror, &nothing);
    if (rc) return rc;
    skg_roi_det_grid G;
    const int tw = nhwc ? SKG_ROI_DET_NT : SKG_ROI_DET_TW, th = nhwc ? SKG_ROI_DET_NT : SKG_ROI_DET_TH;
    const int slab = nhwc ? SKG_ROI_NHWC_SLAB : SKG_ROI_DET_CS;
    G.n_slabs = (C + slab - 1) / slab;
    int64_t blocks = 0;
    for (int l = 0; l < SKG_ROI_MAX_LEVELS; ++l) {
        G.start[l] = (unsigned)blocks;
        G.tiles_x[l] = G.tiles_y[l] = 0;
        if (l >= n_levels) continue;
        if (nhwc && !skg_aligned16(L.feat[l])) return SKG_E_ALIGN;
        G.tiles_x[l] = (L.W[l] + tw - 1) / tw; G.tiles_y[l] = (L.H[l] + th - 1) / th;
        blocks += (int64_t)G.tiles_x[l] * G.tiles_y[l] * n_images * G.n_slabs;
        if (blocks > 0x7fffffffLL) return SKG_E_LIMIT;
    }
    G.start[SKG_ROI_MAX_LEVELS] = (unsigned)blocks;
    g_roi_det_counts[nhwc ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
    skg_roi_with_dtype(grad_dtype, [&](auto d) {
        skg_roi_with_mirror(image_mirror, [&](auto mir) {
            const dim3 grid((unsigned)blocks), wg(256);
            if (nhwc) hipLaunchKernelGGL((skg_roi_align_bwd_det_nhwc_kernel<decltype(d)::value, decltype(mir)::value>), grid, wg, 0, (hipStream_t)stream, L, G, boxes, box_image, n_rois, pooled, sampling, dout, image_mirror);
            else hipLaunchKernelGGL((skg_roi_align_bwd_det_kernel<decltype(d)::value, decltype(mir)::value>), grid, wg, 0, (hipStream_t)stream, L, G, boxes, box_image, n_rois, pooled, sampling, dout, image_mirror);
        });
    });
    return skg_launch_status();
}

#define SKG_ROI_DET_ARGS                                                                                                   \
    void* const* dfeats_host, int grad_dtype, const int32_t* H_host, const int32_t* W_host, const float* scales_host,     \
    int n_levels, int C, int k_min, int k_max, float canonical_scale, int canonical_level, const float* boxes,            \
    const int32_t* box_image, int n_rois, int n_images, int pooled, int sampling, const float* dout
#define SKG_ROI_DET_PASS                                                                                                   \
    dfeats_host, grad_dtype, H_host, W_host, scales_host, n_levels, C, k_min, k_max, canonical_scale, canonical_level,     \
    boxes, box_image, n_rois, n_images, pooled, sampling, dout

extern "C" int skg_roi_align_bwd_det_x(SKG_ROI_DET_ARGS, void* stream) {
    return skg_roi_align_bwd_det(false, SKG_ROI_DET_PASS, nullptr, stream);
}

extern "C" int skg_roi_align_bwd_det_nhwc_x(SKG_ROI_DET_ARGS, void* stream) {
    return skg_roi_align_bwd_det(true, SKG_ROI_DET_PASS, nullptr, stream);
}

// (n_images is part of the deterministic signature already: the siblings add the flags alone)
extern "C" int skg_roi_align_bwd_det_mirror_x(SKG_ROI_DET_ARGS, const int32_t* image_mirror, void* stream) {
    return skg_roi_align_bwd_det(false, SKG_ROI_DET_PASS, image_mirror, stream);
}

extern "C" int skg_roi_align_bwd_det_mirror_nhwc_x(SKG_ROI_DET_ARGS, const int32_t* image_mirror, void* stream) {
    return skg_roi_align_bwd_det(true, SKG_ROI_DET_PASS, image_mirror, stream);
}
