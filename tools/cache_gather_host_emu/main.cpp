// Host emulation of skg_cache.hip: the gather kernel runs on the CPU, one host thread per work-item (the stand-in HIP
// runtime of ../roialign_host_emu), so that AddressSanitizer / UBSan see every table, source and destination access.
// Random ragged sets (rows of 1 .. 25 088 bytes, 16-byte and odd alignments, images without rows, duplicated images, every
// supported dtype pair, a destination shorter than the tables say) are gathered and compared byte for byte with a
// sequential loop written here; sentinel bytes in front of every destination and behind its last row must survive.
// No GPU involved.
//
//   cd tools/cache_gather_host_emu && clang++ -x c++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//       -pthread -I../roialign_host_emu -I../../skghoi_amd/csrc -I../../include main.cpp -o emu && ./emu
// Exit status 0 and "bad 0" on the last line: everything agreed.
#include <hip/hip_runtime.h>
static inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __restrict__
#include "skg_cache.hip"
#include <cstdio>
#include <cstdlib>
#include <random>
thread_local dim3 threadIdx, blockIdx, gridDim;
std::barrier<>* g_barrier;
thread_local const skg_tuning* skg_tls_tuning;
thread_local skg_twin_map skg_tls_twin;

static int esize(int code) { return code == SKG_DTYPE_F32 ? 4 : code == SKG_DTYPE_BYTES ? 1 : 2; }

struct Arr {
    std::vector<int64_t> off; char* src_base; char* src; int64_t row_elems; int sdt, ddt;
    char* dst_base; char* dst; int64_t dst_rows, want_rows;
};

static int run_case(unsigned seed, int n_images, int batch, int n_arrays, bool truncate) {
    std::mt19937 rng(seed);
    auto ri = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    const int64_t order_len = batch + ri(0, 5), first = ri(0, (int)(order_len - batch));
    std::vector<int32_t> order(order_len);
    for (auto& o : order) o = ri(0, n_images - 1);
    if (batch > 2) order[first + 1] = order[first];                  // a duplicated image inside the batch
    static const int64_t ROWS[] = {1, 2, 3, 4, 6, 8, 12, 16, 20, 32, 64, 100, 784, 12544};
    static const int PAIRS[][2] = {{0, 0}, {1, 1}, {2, 2}, {3, 3}, {1, 0}, {2, 0}};
    std::vector<Arr> arrs(n_arrays);
    std::vector<skg_cache_array> desc(n_arrays);
    for (int a = 0; a < n_arrays; ++a) {
        Arr& A = arrs[a];
        const int* pr = PAIRS[ri(0, 5)];
        A.sdt = pr[0]; A.ddt = pr[1];
        A.row_elems = ROWS[ri(0, 13)];
        A.off.assign(n_images + 1, 0);
        for (int i = 0; i < n_images; ++i) A.off[i + 1] = A.off[i] + (ri(0, 3) == 0 ? 0 : ri(0, A.row_elems > 1000 ? 3 : 9));
        const int64_t sbytes = A.off[n_images] * A.row_elems * esize(A.sdt);
        const int mis_s = ri(0, 2) == 0 ? esize(A.sdt) * ri(1, 3) : 0, mis_d = ri(0, 2) == 0 ? esize(A.ddt) * ri(1, 3) : 0;
        A.src_base = (char*)aligned_alloc(16, ((sbytes + mis_s + 15) / 16 + 1) * 16);
        A.src = A.src_base + mis_s;
        for (int64_t k = 0; k < sbytes; ++k) A.src[k] = (char)rng();
        if (A.sdt == SKG_DTYPE_F16)                                  // (no signalling-NaN patterns: the host's conversion may quiet them)
            for (int64_t k = 0; k < sbytes / 2; ++k) {
                uint16_t* h = (uint16_t*)A.src + k;
                if ((*h & 0x7C00u) == 0x7C00u) *h &= 0xFC00u;
            }
        A.want_rows = 0;
        for (int b = 0; b < batch; ++b) { const int i = order[first + b]; A.want_rows += A.off[i + 1] - A.off[i]; }
        A.dst_rows = truncate && A.want_rows > 1 ? A.want_rows - 1 : A.want_rows;
        const int64_t dbytes = A.dst_rows * A.row_elems * esize(A.ddt);
        // the start of the destination gets the wanted (mis)alignment; sentinels in front of it and behind its last row
        const int64_t lead = 16 + mis_d;
        A.dst_base = (char*)aligned_alloc(16, ((lead + dbytes + 15) / 16) * 16 + 16);
        A.dst = A.dst_base + lead;
        memset(A.dst_base, 0x5A, ((lead + dbytes + 15) / 16) * 16 + 16);
        desc[a] = skg_cache_array{A.src, A.off.data(), A.row_elems, A.sdt, 0, A.dst, A.ddt, 0, A.dst_rows};
    }
    const int rc = skg_cache_gather_x(desc.data(), n_arrays, order.data(), order_len, first, batch, nullptr);
    int bad = rc != 0;
    for (int a = 0; a < n_arrays; ++a) {
        Arr& A = arrs[a];
        const int64_t sb = A.row_elems * esize(A.sdt), db = A.row_elems * esize(A.ddt);
        std::vector<char> want(A.dst_rows * db + 1, 0);
        int64_t row = 0;
        for (int b = 0; b < batch; ++b) {
            const int i = order[first + b];
            for (int64_t r = A.off[i]; r < A.off[i + 1]; ++r, ++row) {
                if (row >= A.dst_rows) continue;
                const char* s = A.src + r * sb;
                char* d = want.data() + row * db;
                if (A.sdt == A.ddt) memcpy(d, s, sb);
                else
                    for (int64_t e = 0; e < A.row_elems; ++e) {
                        uint16_t h; memcpy(&h, s + 2 * e, 2);
                        float f;
                        if (A.sdt == SKG_DTYPE_BF16) f = __uint_as_float((uint32_t)h << 16);
                        else { _Float16 x; memcpy(&x, &h, 2); f = (float)x; }
                        memcpy(d + 4 * e, &f, 4);
                    }
            }
        }
        if (memcmp(want.data(), A.dst, A.dst_rows * db)) { ++bad; printf("  array %d differs (dtypes %d -> %d, row %lld)\n", a, A.sdt, A.ddt, (long long)A.row_elems); }
        const int64_t lead = A.dst - A.dst_base;
        for (int64_t k = 0; k < lead; ++k) if (A.dst_base[k] != 0x5A) { ++bad; printf("  array %d: write in front of dst\n", a); break; }
        for (int64_t k = 0; k < 16; ++k) if (A.dst[A.dst_rows * db + k] != 0x5A) { ++bad; printf("  array %d: write behind dst_rows\n", a); break; }
        free(A.src_base); free(A.dst_base);
    }
    printf("case seed %u images %d batch %d arrays %d truncate %d: %s\n", seed, n_images, batch, n_arrays, (int)truncate, bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    bad += run_case(1, 1, 1, 1, false);
    bad += run_case(2, 5, 4, 10, false);
    bad += run_case(3, 9, 7, SKG_CACHE_MAX_ARRAYS, false);
    bad += run_case(4, 3, 4, 6, true);
    bad += run_case(5, 40, SKG_CACHE_MAX_BATCH, 3, false);
    for (unsigned s = 10; s < 22; ++s) bad += run_case(s, 2 + s % 7, 1 + s % 9, 1 + s % 11, s % 3 == 0);
    printf("bad %d\n", bad);
    return bad != 0;
}
