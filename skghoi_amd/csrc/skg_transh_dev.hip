// skg_transh_dev.hip -- TransH tables and training negatives generated on the device, keyed by the content of the image
// (include/skghoi.h: the rule; skg_transh_philox.h: its one implementation).  Three small kernels and their host twins.
#include <algorithm>
#include <vector>
#include "skg_common.h"
#include "skg_transh_philox.h"

namespace {

constexpr int ENT_ELEMS = SKG_TRANSH_ENT * SKG_TRANSH_DIM;           // 4000: a multiple of 4
constexpr int ENT_QUADS = ENT_ELEMS / 4;

// ------------------------------------------------------------------------------------------------ keys
// One wavefront per image.  The hash is serial, its inputs are not: the lanes fetch the image's 6 n node words side by side
// into LDS (one thread reading them one after the other pays a memory round trip per word: ~300 of them at 48 nodes), then
// lane 0 folds them in order.  An image with more nodes than the head ever selects is folded from memory.
__global__ __launch_bounds__(64) void skg_transh_keys_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int64_t* __restrict__ labels,
                                                             const skg_image_meta* __restrict__ meta, uint64_t seed,
                                                             uint64_t salt, uint64_t* __restrict__ keys) {
    __shared__ uint32_t words[6 * SKG_MAX_NODES];
    const int a = blockIdx.x, lane = threadIdx.x;
    const skg_image_meta mt = meta[a];
    const float* b = boxes + 4 * (int64_t)mt.box_off;
    const float* s = scores + mt.box_off;
    const int64_t* l = labels + mt.box_off;
    const bool staged = mt.n <= SKG_MAX_NODES;
    if (staged)
        for (int i = lane; i < 6 * mt.n; i += 64) words[i] = skg_transh_node_word(b, s, l, i);
    __syncthreads();
    if (lane != 0) return;
    keys[a] = staged ? skg_transh_image_key(seed, salt, mt.img_h, mt.img_w, mt.n_h, mt.n, [&](int i) { return words[i]; })
                     : skg_transh_image_key(seed, salt, mt.img_h, mt.img_w, mt.n_h, mt.n,
                                            [&](int i) { return skg_transh_node_word(b, s, l, i); });
}

// ------------------------------------------------------------------------------------------------ tables
// Which table, which quad of it and where it goes, for quad q of an image's [ent | rel | nrm] quads.
struct QuadSlot { float* dst; int n_el; uint32_t j, s; float a; };

__host__ __device__ inline QuadSlot quad_slot(int q, int64_t image, int K, float a_ent, float a_rel, float* ent, float* rel,
                                              float* nrm) {
    const int n_r = K * SKG_TRANSH_DIM, qr = (n_r + 3) / 4;
    if (q < ENT_QUADS) return {ent + image * ENT_ELEMS, ENT_ELEMS, (uint32_t)q, 0u, a_ent};
    q -= ENT_QUADS;
    if (q < qr) return {rel + image * n_r, n_r, (uint32_t)q, 1u, a_rel};
    return {nrm + image * n_r, n_r, (uint32_t)(q - qr), 2u, a_rel};
}

// One thread = one Philox quad = up to four floats.  A table of an odd K has 50 K = 2 (mod 4) elements: its last quad
// stores two, and the tables of every second image start 8 bytes off a 16-byte boundary.
__global__ __launch_bounds__(256) void skg_transh_fill_kernel(const uint64_t* __restrict__ keys, int quads, int blocks_per_image,
                                                              int K, float a_ent, float a_rel, float* __restrict__ ent,
                                                              float* __restrict__ rel, float* __restrict__ nrm) {
    const int image = blockIdx.x / blocks_per_image;
    const int q = (blockIdx.x - image * blocks_per_image) * 256 + threadIdx.x;
    if (q >= quads) return;
    const QuadSlot t = quad_slot(q, image, K, a_ent, a_rel, ent, rel, nrm);
    float v[4];
    skg_transh_quad(keys[image], t.j, t.s, t.a, v);
    float* p = t.dst + 4 * (int64_t)t.j;
    const int left = t.n_el - 4 * (int)t.j;
    if (left >= 4 && skg_aligned16_dev(p)) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (left >= 4 && (((uintptr_t)p) & 7u) == 0) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2*>(p + 2) = make_float2(v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) p[i] = v[i];
    }
}

// ------------------------------------------------------------------------------------------------ negatives
// The m smallest of the n composites c(r) of an image, ascending.  One workgroup per image.  Every sweep over the ranks
// regenerates the composites -- 10 rounds of integer ALU per four ranks, nothing is read from memory -- and a sweep over ~10^5
// ranks is what this kernel costs, so the usual case takes ONE:
//   short cut  the Philox words are uniform, so the m-th smallest lies near m / n of their range: the composites whose word is
//              at or below a cut a little above that (m + 8 sqrt(m) + 16 expected) are collected in LDS.  If at least m and
//              at most NEG_CAND came, the sample is among them: sort them, emit the first m.  Any cut gives the same answer;
//              a cut that caught too few (rarer than one sweep in 10^10) or too many (m near n, m above NEG_CAND) falls through to
//   general    a radix select, most significant digit first (11 / 11 / 10 bits of the word, then of the rank): an LDS
//              histogram of the digit over the composites that share the prefix found so far, a scan by the first wavefront,
//              the digit of the m-th smallest; it stops as soon as the chosen bin holds exactly what is still needed (the rank
//              digits are visited only to break a tie between equal words).  The composites at or below that bound (exactly
//              m: they are distinct) are gathered into the image's slice of perm_out and sorted there.
// The sort is a bitonic network in its mirror form: entries past the end count as +infinity and never move.
constexpr int NEG_THREADS = 1024;
constexpr int NEG_BINS = 2048;
constexpr int NEG_CAND = 4096;

__device__ __forceinline__ void cmp_swap(unsigned long long* v, int lo, int hi) {
    const unsigned long long x = v[lo], y = v[hi];
    if (x > y) { v[lo] = y; v[hi] = x; }
}

// v[0, m) ascending, by the whole workgroup (v in LDS or in global memory); every thread of it must call.
__device__ void sort_ascending(unsigned long long* v, int m, int tid) {
    int span = 1;
    while (span < m) span <<= 1;
    for (int k = 2; k <= span; k <<= 1) {
        for (int t = tid; t < span / 2; t += NEG_THREADS) {          // mirror step: i against the far end of its block
            const int blk = t / (k / 2), off = t % (k / 2);
            const int lo = blk * k + off, hi = blk * k + k - 1 - off;
            if (hi < m) cmp_swap(v, lo, hi);
        }
        __threadfence_block();
        __syncthreads();
        for (int j = k / 4; j > 0; j >>= 1) {
            for (int t = tid; t < span / 2; t += NEG_THREADS) {
                const int lo = (t / j) * 2 * j + t % j, hi = lo + j;
                if (hi < m) cmp_swap(v, lo, hi);
            }
            __threadfence_block();
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(NEG_THREADS) void skg_transh_negatives_kernel(const uint64_t* __restrict__ keys,
                                                                           const int32_t* __restrict__ n_neg,
                                                                           const int32_t* __restrict__ pos_off,
                                                                           int64_t* __restrict__ perm_out) {
    __shared__ unsigned long long cand[NEG_CAND];
    __shared__ uint32_t hist[NEG_BINS];
    __shared__ uint32_t sel[3];                 // chosen bin, composites in the bins below it, composites in it
    __shared__ uint32_t taken;
    const int a = blockIdx.x, tid = threadIdx.x;
    const int n = n_neg[a], o0 = pos_off[a];
    const int m = min(pos_off[a + 1] - o0, n);  // (m <= n is the caller's contract; never write past n ranks)
    if (m <= 0) return;
    const uint64_t key = keys[a];
    const uint32_t nq = ((uint32_t)n + 3u) / 4u;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(perm_out) + o0;

    // ---- short cut: one sweep, the candidates below the cut
    const double expect = (double)m + 8.0 * sqrt((double)m) + 16.0;
    const uint32_t cut = expect >= (double)n ? 0xffffffffu : (uint32_t)(expect / (double)n * 4294967296.0);
    if (tid == 0) taken = 0;
    __syncthreads();
    for (uint32_t q = tid; q < nq; q += NEG_THREADS) {
        uint64_t c[4];
        skg_transh_neg_quad(key, q, c);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4u * q + i < (uint32_t)n && (uint32_t)(c[i] >> 32) <= cut) {
                const uint32_t slot = atomicAdd(&taken, 1u);
                if (slot < (uint32_t)NEG_CAND) cand[slot] = c[i];
            }
    }
    __syncthreads();
    const uint32_t caught = taken;              // (the same in every thread: read behind the barrier)
    if (caught >= (uint32_t)m && caught <= (uint32_t)NEG_CAND) {
        sort_ascending(cand, (int)caught, tid);
        for (int i = tid; i < m; i += NEG_THREADS) out[i] = cand[i] & 0xffffffffull;
        return;
    }

    // ---- general: radix select of the m-th smallest composite
    uint64_t prefix = 0, known = 0, bound = 0;  // bits of the m-th smallest found so far, their mask, the final bound
    uint32_t need = (uint32_t)m;
    const int shifts[6] = {53, 42, 32, 21, 10, 0}, widths[6] = {11, 11, 10, 11, 11, 10};
    for (int pass = 0; pass < 6; ++pass) {
        const int shift = shifts[pass];
        const uint32_t dmask = (1u << widths[pass]) - 1u;
        for (int b = tid; b < NEG_BINS; b += NEG_THREADS) hist[b] = 0;
        __syncthreads();
        for (uint32_t q = tid; q < nq; q += NEG_THREADS) {
            uint64_t c[4];
            skg_transh_neg_quad(key, q, c);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4u * q + i < (uint32_t)n && (c[i] & known) == prefix) atomicAdd(&hist[(uint32_t)(c[i] >> shift) & dmask], 1u);
        }
        __syncthreads();
        if (tid < 64) {                         // the first wavefront: 32 bins per lane, a scan over the lanes
            uint32_t mine = 0;
            for (int b = 0; b < NEG_BINS / 64; ++b) mine += hist[tid * (NEG_BINS / 64) + b];
            uint32_t incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_up(incl, off, 64);
                if (tid >= off) incl += up;
            }
            uint32_t below = incl - mine;
            if (below < need && need <= incl) { // exactly one lane: the bin of the need-th smallest lies in its range
                for (int b = 0; b < NEG_BINS / 64; ++b) {
                    const uint32_t h = hist[tid * (NEG_BINS / 64) + b];
                    if (need <= below + h) { sel[0] = tid * (NEG_BINS / 64) + b; sel[1] = below; sel[2] = h; break; }
                    below += h;
                }
            }
        }
        __syncthreads();
        need -= sel[1];
        prefix |= (uint64_t)sel[0] << shift;
        known |= (uint64_t)dmask << shift;
        bound = prefix | ~known;                // everything that shares the prefix
        if (sel[2] == need) break;              // ... is wanted: done
    }
    __syncthreads();                            // (every thread has read `taken` above before it is cleared)
    if (tid == 0) taken = 0;
    __syncthreads();
    for (uint32_t q = tid; q < nq; q += NEG_THREADS) {
        uint64_t c[4];
        skg_transh_neg_quad(key, q, c);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4u * q + i < (uint32_t)n && c[i] <= bound) {
                const uint32_t slot = atomicAdd(&taken, 1u);
                if (slot < (uint32_t)m) out[slot] = c[i];
            }
    }
    __threadfence_block();
    __syncthreads();
    sort_ascending(out, m, tid);
    for (int i = tid; i < m; i += NEG_THREADS) out[i] = out[i] & 0xffffffffull;
}

}  // namespace

extern "C" int skg_transh_keys_u64(const float* boxes, const float* scores, const int64_t* labels, const skg_image_meta* meta,
                                   int n_active, uint64_t seed, uint64_t salt, uint64_t* keys_out, void* stream) {
    if (n_active < 0) return SKG_E_ARG;
    if (n_active == 0) return 0;
    if (!boxes || !scores || !labels || !meta || !keys_out) return SKG_E_ARG;
    hipLaunchKernelGGL(skg_transh_keys_kernel, dim3(n_active), dim3(64), 0, (hipStream_t)stream, boxes, scores, labels, meta,
                       seed, salt, keys_out);
    return skg_launch_status();
}

extern "C" int skg_transh_keys_host_u64(const float* boxes_host, const float* scores_host, const int64_t* labels_host,
                                        const skg_image_meta* meta_host, int n_active, uint64_t seed, uint64_t salt,
                                        uint64_t* keys_host) {
    if (n_active < 0) return SKG_E_ARG;
    if (n_active == 0) return 0;
    if (!boxes_host || !scores_host || !labels_host || !meta_host || !keys_host) return SKG_E_ARG;
    for (int a = 0; a < n_active; ++a) {
        const skg_image_meta& mt = meta_host[a];
        if (mt.n < 0 || mt.box_off < 0) return SKG_E_ARG;
        const float* b = boxes_host + 4 * (int64_t)mt.box_off;
        const float* s = scores_host + mt.box_off;
        const int64_t* l = labels_host + mt.box_off;
        keys_host[a] = skg_transh_image_key(seed, salt, mt.img_h, mt.img_w, mt.n_h, mt.n,
                                            [&](int i) { return skg_transh_node_word(b, s, l, i); });
    }
    return 0;
}

extern "C" int skg_transh_philox_host_u32(const uint32_t* counter_host, const uint32_t* key_host, uint32_t* out_host) {
    if (!counter_host || !key_host || !out_host) return SKG_E_ARG;
    skg_philox4x32_10(counter_host[0], counter_host[1], counter_host[2], counter_host[3], key_host[0], key_host[1], out_host);
    return 0;
}

static int fill_args_ok(const void* keys, int n_active, int K, int need_relations, const void* ent, const void* rel,
                        const void* nrm) {
    if (n_active < 0 || K < 1) return SKG_E_ARG;
    if (n_active > 0 && (!keys || !ent || (need_relations && (!rel || !nrm)))) return SKG_E_ARG;
    if (K > (1 << 20)) return SKG_E_LIMIT;      // keeps the quad arithmetic inside int32
    return 0;
}

extern "C" int skg_transh_fill_f32(const uint64_t* keys, int n_active, int K, int need_relations, float a_ent, float a_rel,
                                   float* ent, float* rel, float* nrm, void* stream) {
    const int rc = fill_args_ok(keys, n_active, K, need_relations, ent, rel, nrm);
    if (rc || n_active == 0) return rc;
    const int quads = ENT_QUADS + (need_relations ? 2 * ((K * SKG_TRANSH_DIM + 3) / 4) : 0);
    const int bpi = (quads + 255) / 256;
    if ((int64_t)bpi * n_active > 0x7fffffffll) return SKG_E_LIMIT;
    hipLaunchKernelGGL(skg_transh_fill_kernel, dim3(bpi * n_active), dim3(256), 0, (hipStream_t)stream, keys, quads, bpi, K,
                       a_ent, a_rel, ent, rel, nrm);
    return skg_launch_status();
}

extern "C" int skg_transh_fill_host_f32(const uint64_t* keys_host, int n_active, int K, int need_relations, float a_ent,
                                        float a_rel, float* ent_host, float* rel_host, float* nrm_host) {
    const int rc = fill_args_ok(keys_host, n_active, K, need_relations, ent_host, rel_host, nrm_host);
    if (rc) return rc;
    const int quads = ENT_QUADS + (need_relations ? 2 * ((K * SKG_TRANSH_DIM + 3) / 4) : 0);
    for (int a = 0; a < n_active; ++a)
        for (int q = 0; q < quads; ++q) {
            const QuadSlot t = quad_slot(q, a, K, a_ent, a_rel, ent_host, rel_host, nrm_host);
            float v[4];
            skg_transh_quad(keys_host[a], t.j, t.s, t.a, v);
            for (int i = 0; i < 4 && 4 * (int)t.j + i < t.n_el; ++i) t.dst[4 * (int64_t)t.j + i] = v[i];
        }
    return 0;
}

extern "C" int skg_transh_negatives_i64(const uint64_t* keys, int n_active, const int32_t* n_neg, const int32_t* pos_off,
                                        int64_t* perm_out, void* stream) {
    if (n_active < 0) return SKG_E_ARG;
    if (n_active == 0) return 0;
    if (!keys || !n_neg || !pos_off || !perm_out) return SKG_E_ARG;
    hipLaunchKernelGGL(skg_transh_negatives_kernel, dim3(n_active), dim3(NEG_THREADS), 0, (hipStream_t)stream, keys, n_neg,
                       pos_off, perm_out);
    return skg_launch_status();
}

extern "C" int skg_transh_negatives_host_i64(const uint64_t* keys_host, int n_active, const int32_t* n_neg_host,
                                             const int32_t* pos_off_host, int64_t* perm_out_host) {
    if (n_active < 0) return SKG_E_ARG;
    if (n_active == 0) return 0;
    if (!keys_host || !n_neg_host || !pos_off_host) return SKG_E_ARG;
    for (int a = 0; a < n_active; ++a) {
        const int64_t m = (int64_t)pos_off_host[a + 1] - pos_off_host[a];
        if (n_neg_host[a] < 0 || m < 0 || m > n_neg_host[a] || (m > 0 && !perm_out_host)) return SKG_E_ARG;
    }
    std::vector<uint64_t> c;
    for (int a = 0; a < n_active; ++a) {
        const uint32_t n = (uint32_t)n_neg_host[a], nq = (n + 3u) / 4u;
        const int64_t m = (int64_t)pos_off_host[a + 1] - pos_off_host[a];
        if (m == 0) continue;
        c.resize((size_t)nq * 4);
        for (uint32_t q = 0; q < nq; ++q) skg_transh_neg_quad(keys_host[a], q, c.data() + 4 * (size_t)q);
        c.resize(n);
        std::partial_sort(c.begin(), c.begin() + m, c.end());
        for (int64_t i = 0; i < m; ++i) perm_out_host[pos_off_host[a] + i] = (int64_t)(c[i] & 0xffffffffull);
    }
    return 0;
}
