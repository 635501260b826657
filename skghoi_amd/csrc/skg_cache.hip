// Batch gather out of a device-resident feature set (include/skghoi.h: skg_cache_gather_x; skghoi_amd/resident.py).
// One launch assembles every ragged array of a batch -- pooled box features (copied or widened to fp32), global features,
// detections, targets -- in the sampler's order.  Memory-bound: a 4-image batch of 30-box images moves 3 MB (bf16 -> fp32:
// 1.5 MB read, 3 MB written).
#include "skg_common.h"

namespace {

enum { MODE_COPY16 = 0, MODE_COPY_UNIT, MODE_F16_16, MODE_BF16_16, MODE_F16_1, MODE_BF16_1 };

struct CacheArr {
    const char* src; const int64_t* off; char* dst;
    int64_t src_row_bytes, dst_row_bytes;
    int64_t dst_rows;            // rows the host counted for this batch: no store at or behind it
    int32_t pieces_per_row;      // src_row_bytes / piece bytes
    int32_t mode;
    int32_t unit;                // MODE_COPY_UNIT: bytes per piece (8, 4, 2 or 1)
    int32_t pad;
};
struct CacheArgs { CacheArr a[SKG_CACHE_MAX_ARRAYS]; int32_t n; };

__device__ __forceinline__ void widen8(const uint4 v, const bool bf16, float4& lo, float4& hi) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    float f[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (bf16) {
            f[2 * k] = __uint_as_float(w[k] << 16);
            f[2 * k + 1] = __uint_as_float(w[k] & 0xFFFF0000u);
        } else {
            f[2 * k] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[k] & 0xFFFFu));
            f[2 * k + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[k] >> 16));
        }
    }
    lo = make_float4(f[0], f[1], f[2], f[3]);
    hi = make_float4(f[4], f[5], f[6], f[7]);
}

__global__ __launch_bounds__(256) void cache_gather_kernel(const CacheArgs A, const int32_t* __restrict__ order,
                                                           const int64_t first, const int batch) {
    __shared__ int32_t tab[SKG_CACHE_MAX_ARRAYS][SKG_CACHE_MAX_BATCH + 1];     // rows in front of slot b, per array
    __shared__ int32_t img[SKG_CACHE_MAX_BATCH];
    __shared__ int64_t tile0[SKG_CACHE_MAX_ARRAYS + 1];                        // first tile of each array
    const int tid = threadIdx.x;
    if (tid < batch) img[tid] = order[first + tid];
    __syncthreads();
    for (int a = 0; a < A.n; ++a) {
        const int64_t* off = A.a[a].off;
        if (tid < batch) {
            const int64_t i = img[tid];
            const int64_t c = off[i + 1] - off[i];
            tab[a][tid + 1] = (int32_t)(c < 0 ? 0 : (c > 0x7FFFFFFF ? 0x7FFFFFFF : c));
        }
    }
    __syncthreads();
    if (tid < A.n) {                                   // one lane per array: at most 256 LDS adds
        int64_t s = 0;
        tab[tid][0] = 0;
        for (int b = 1; b <= batch; ++b) {
            s += tab[tid][b];
            tab[tid][b] = (int32_t)(s > 0x7FFFFFFF ? 0x7FFFFFFF : s);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int64_t t = 0;
        for (int a = 0; a < A.n; ++a) {
            tile0[a] = t;
            const int64_t rows = min((int64_t)tab[a][batch], A.a[a].dst_rows);
            t += (rows * A.a[a].pieces_per_row + 255) >> 8;
        }
        tile0[A.n] = t;
    }
    __syncthreads();
    const int64_t tiles = tile0[A.n];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int a = 0;
        while (t >= tile0[a + 1]) ++a;                 // (empty arrays have tile0[a] == tile0[a + 1])
        a = __builtin_amdgcn_readfirstlane(a);         // workgroup-uniform: the descriptor is read with scalar loads
        const CacheArr& R = A.a[a];
        const int64_t rows = min((int64_t)tab[a][batch], R.dst_rows);
        const int64_t piece = ((t - tile0[a]) << 8) + tid;
        const int64_t pieces = rows * R.pieces_per_row;
        if (piece >= pieces) continue;
        const int32_t row = pieces <= 0x7FFFFFFF ? (int32_t)((uint32_t)piece / (uint32_t)R.pieces_per_row)
                                                 : (int32_t)(piece / R.pieces_per_row);
        const int64_t p = piece - (int64_t)row * R.pieces_per_row;
        int lo = 0, hi = batch - 1;                    // the last slot b with tab[a][b] <= row (slots without rows are passed over)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[a][mid] <= row) lo = mid; else hi = mid - 1;
        }
        const int64_t srow = R.off[img[lo]] + (row - tab[a][lo]);
        const char* s = R.src + srow * R.src_row_bytes;
        char* d = R.dst + (int64_t)row * R.dst_row_bytes;
        switch (R.mode) {
        case MODE_COPY16:
            reinterpret_cast<uint4*>(d)[p] = reinterpret_cast<const uint4*>(s)[p];
            break;
        case MODE_COPY_UNIT:
            if (R.unit == 8) reinterpret_cast<uint2*>(d)[p] = reinterpret_cast<const uint2*>(s)[p];
            else if (R.unit == 4) reinterpret_cast<uint32_t*>(d)[p] = reinterpret_cast<const uint32_t*>(s)[p];
            else if (R.unit == 2) reinterpret_cast<uint16_t*>(d)[p] = reinterpret_cast<const uint16_t*>(s)[p];
            else d[p] = s[p];
            break;
        case MODE_F16_16:
        case MODE_BF16_16: {
            float4 x, y;
            widen8(reinterpret_cast<const uint4*>(s)[p], R.mode == MODE_BF16_16, x, y);
            reinterpret_cast<float4*>(d)[2 * p] = x;
            reinterpret_cast<float4*>(d)[2 * p + 1] = y;
            break;
        }
        case MODE_F16_1:
            reinterpret_cast<float*>(d)[p] = (float)__builtin_bit_cast(_Float16, reinterpret_cast<const uint16_t*>(s)[p]);
            break;
        default:                                       // MODE_BF16_1
            reinterpret_cast<float*>(d)[p] = __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(s)[p] << 16);
            break;
        }
    }
}

inline int elem_bytes(int code) { return code == SKG_DTYPE_F32 ? 4 : code == SKG_DTYPE_BYTES ? 1 : 2; }

}  // namespace

extern "C" int skg_sizeof_cache_array(void) { return (int)sizeof(skg_cache_array); }

extern "C" int skg_cache_gather_x(const skg_cache_array* arrays, int n_arrays, const int32_t* order, int64_t order_len,
                                  int64_t first, int batch, void* stream) {
    if (!arrays || !order || n_arrays < 1 || n_arrays > SKG_CACHE_MAX_ARRAYS || batch < 1 || batch > SKG_CACHE_MAX_BATCH ||
        first < 0 || order_len < 0 || first > order_len - batch)
        return SKG_E_ARG;
    CacheArgs A = {};
    A.n = n_arrays;
    int64_t tiles = 0;
    for (int k = 0; k < n_arrays; ++k) {
        const skg_cache_array& in = arrays[k];
        CacheArr& o = A.a[k];
        if (!in.src || !in.src_off || !in.dst || in.row_elems < 1 || in.dst_rows < 0 || in.src_dtype < 0 ||
            in.src_dtype > SKG_DTYPE_BYTES || in.dst_dtype < 0 || in.dst_dtype > SKG_DTYPE_BYTES)
            return SKG_E_ARG;
        const bool same = in.src_dtype == in.dst_dtype;
        const bool widen = in.dst_dtype == SKG_DTYPE_F32 && (in.src_dtype == SKG_DTYPE_F16 || in.src_dtype == SKG_DTYPE_BF16);
        if (!same && !widen) return SKG_E_ARG;
        if (in.dst_rows > 0x7FFFFFFF) return SKG_E_LIMIT;
        const uintptr_t sp = (uintptr_t)in.src, dp = (uintptr_t)in.dst;
        if (sp % elem_bytes(in.src_dtype) || dp % elem_bytes(in.dst_dtype)) return SKG_E_ALIGN;
        o.src = (const char*)in.src; o.off = in.src_off; o.dst = (char*)in.dst;
        o.src_row_bytes = in.row_elems * elem_bytes(in.src_dtype);
        o.dst_row_bytes = in.row_elems * elem_bytes(in.dst_dtype);
        o.dst_rows = in.dst_rows;
        o.pad = 0;
        const bool vec = o.src_row_bytes % 16 == 0 && sp % 16 == 0 && dp % 16 == 0;
        int64_t piece;
        if (same) {
            o.unit = 16;
            if (!vec)
                for (o.unit = 8; o.unit > 1 && (o.src_row_bytes % o.unit || sp % o.unit || dp % o.unit); o.unit >>= 1) {}
            o.mode = vec ? MODE_COPY16 : MODE_COPY_UNIT;
            piece = o.unit;
        } else {
            const bool bf = in.src_dtype == SKG_DTYPE_BF16;
            o.mode = vec ? (bf ? MODE_BF16_16 : MODE_F16_16) : (bf ? MODE_BF16_1 : MODE_F16_1);
            o.unit = vec ? 16 : 2;
            piece = o.unit;
        }
        const int64_t ppr = o.src_row_bytes / piece;
        if (ppr > 0x7FFFFFFF) return SKG_E_LIMIT;
        o.pieces_per_row = (int32_t)ppr;
        tiles += (in.dst_rows * ppr + 255) >> 8;
    }
    if (tiles == 0) return 0;
    const int grid = (int)(tiles < 2048 ? tiles : 2048);
    hipLaunchKernelGGL(cache_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, A, order, first, batch);
    return skg_launch_status();
}
