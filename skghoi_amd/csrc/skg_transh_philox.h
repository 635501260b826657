// The device-generated TransH tables (include/skghoi.h, "TransH tables keyed by image content"): the ONE statement of the
// rule in code -- Philox4x32-10, the image key, the table value and the negatives' composite -- shared by the kernels and
// their host twins (skg_transh_dev.hip).  Integer arithmetic and two fp32 roundings: host and device agree bit for bit.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SKG_HD __host__ __device__ __forceinline__
#else
#define SKG_HD inline
#endif

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between them.
SKG_HD void skg_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

SKG_HD uint32_t skg_f32_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
SKG_HD uint64_t skg_key_mix(uint64_t h, uint32_t w) { return (h ^ (uint64_t)w) * 0x100000001b3ull; }     // FNV-1a over 32-bit words

// Word i of an image's 6 n node words: per selected node, in the head's node order, the bits of x1, y1, x2, y2, the bits of
// the score, the low word of the label.  boxes [n, 4], scores [n], labels [n]: the image's rows of the packed selection.
SKG_HD uint32_t skg_transh_node_word(const float* boxes, const float* scores, const int64_t* labels, int32_t i) {
    const int32_t node = i / 6, c = i - 6 * node;
    if (c < 4) return skg_f32_bits(boxes[4 * (int64_t)node + c]);
    return c == 4 ? skg_f32_bits(scores[node]) : (uint32_t)(uint64_t)labels[node];
}

// Key of one image: seed, salt, the image size, the node counts and the 6 n node words (node_word(i), i ascending), finished
// with splitmix64's finaliser.
template <class NodeWord>
SKG_HD uint64_t skg_transh_image_key(uint64_t seed, uint64_t salt, float img_h, float img_w, int32_t n_h, int32_t n,
                                     NodeWord node_word) {
    uint64_t h = 0xcbf29ce484222325ull;
    h = skg_key_mix(h, (uint32_t)seed); h = skg_key_mix(h, (uint32_t)(seed >> 32));
    h = skg_key_mix(h, (uint32_t)salt); h = skg_key_mix(h, (uint32_t)(salt >> 32));
    h = skg_key_mix(h, skg_f32_bits(img_h)); h = skg_key_mix(h, skg_f32_bits(img_w));
    h = skg_key_mix(h, (uint32_t)n_h); h = skg_key_mix(h, (uint32_t)n);
    for (int32_t i = 0; i < 6 * n; ++i) h = skg_key_mix(h, node_word(i));
    h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27; h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}

// One table value from one Philox word: a 24-bit uniform in [0, 1) mapped to [-a, a).  Multiply and add round separately.
SKG_HD float skg_transh_value(uint32_t x, float a) {
#pragma clang fp contract(off)
    const float u = (float)(x >> 8) * 5.9604644775390625e-08f;      // * 2^-24, exact
    const float t = u * (2.0f * a);
    return t + (-a);
}

// The four values of quad j of table s (0 ent, 1 rel, 2 nrm): elements 4 j .. 4 j + 3.
SKG_HD void skg_transh_quad(uint64_t key, uint32_t j, uint32_t s, float a, float v[4]) {
    uint32_t w[4];
    skg_philox4x32_10(j, s, 0u, 0u, (uint32_t)key, (uint32_t)(key >> 32), w);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = skg_transh_value(w[i], a);
}

// Composites of the four zero-cell ranks 4 q .. 4 q + 3 (table 3): the sampled negatives are the ranks with the smallest.
SKG_HD void skg_transh_neg_quad(uint64_t key, uint32_t q, uint64_t c[4]) {
    uint32_t w[4];
    skg_philox4x32_10(q, 3u, 0u, 0u, (uint32_t)key, (uint32_t)(key >> 32), w);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = ((uint64_t)w[i] << 32) | (uint64_t)(4u * q + (uint32_t)i);
}
