// skg_eval.hip -- the evaluator behind the head's results on the device: 600-way HOI mapping, box-pair association at
// IoU 0.5, and 11-point AP per interaction class.
//
// Reference: utils.py:148-198 (`test`): per image, interactions = object_n_verb_to_interaction[object][verb]
// (hicodet/hicodet.py:139-153), then for every predicted interaction class pocket's BoxPairAssociation(min_iou = 0.5)
// against the ground-truth pairs of that class -- a detection matches the ground-truth pair of largest
// min(IoU_human, IoU_object) if that reaches min_iou, and among the detections matched to one ground-truth pair the
// highest-scoring one is the true positive -- and pocket's DetectionAPMeter(600, algorithm = '11P').  The reference does
// this per detection in Python on the CPU, one image per forward; pocket is a third-party package absent from the image
// (parity is unpinned at that boundary; oracle/eval_oracle.py restates the published semantics loop by loop).
//
//   skg_eval_associate_f32 : one workgroup per image.  Every lane takes detections, scans the image's ground-truth pairs of
//                            its class (a few dozen at most), and bids for its match with a 64-bit key (score, then lower
//                            index) by LDS atomicMax; the winners are the true positives.
//   skg_eval_ap11_f64      : one workgroup per class over the globally sorted detections (class ascending, score
//                            descending, stable): running true-positive count by block scans, eleven running maxima of
//                            the precision, float64 like pocket.
//   skg_eval_known_object_u8 : HICO-DET's Known Object setting, launched behind the association: one workgroup per image,
//                            the object categories of its ground truth as an LDS bit mask, one keep flag per cell.
//   skg_eval_hoi_errors_u8 : the error breakdown of the Default setting (this project's own definition), launched behind the
//                            association: one workgroup per image, one flag word per ground-truth pair in LDS, one category
//                            per cell and one status per ground-truth pair.
//
// V-COCO (role AP, scenarios 1 and 2; the published toolkit's `_do_role_eval`, restated in include/skghoi.h -- the toolkit is
// outside the reference tree, parity unpinned at that boundary):
//
//   skg_eval_vcoco_match_f32 : one workgroup per (image, class).  The image's persons and their ignore flags sit in LDS;
//                              every lane takes cells of the class, finds the person of largest overlap and bids for it
//                              with the same 64-bit key, once per scenario (two LDS key arrays).
//   skg_eval_ap_voc_f64      : one workgroup per class over the same sorted labels: the class's true-positive total by a
//                              block reduction, then one backward pass of reversed block scans carrying the suffix
//                              true-positive count and the suffix maximum of the precision; float64.
//
// Object detections (the boxes that go into the cache; hicodet/detections/eval_detections.py:91-127, restated in
// include/skghoi.h -- torchvision's tie order, pocket's BoxAssociation and 'INT' are outside the image, parity unpinned there):
//
//   skg_eval_det_match_f32   : one workgroup per image.  The image's 2G ground-truth boxes sit in LDS; class-wise greedy NMS
//                              over them in index order (the preprocess kernel's coordinate trick and barrier order), then
//                              every lane takes detections, finds the kept box of its class of largest IoU and bids for it
//                              with the same 64-bit key.
//   skg_eval_pair_cover_u8   : one workgroup per image, one lane per ground-truth pair, the detections through LDS in chunks:
//                              is the human box and the object box of the pair covered by two different detections.
//
// Pair NMS over the head's scored cells (opt-in post-processing, not the reference's; the published PNMS idea restated in
// include/skghoi.h -- parity unpinned):
//
//   skg_hoi_pair_nms_u8      : one workgroup per image over the cells sorted by (group, score): the group starts compacted
//                              into an LDS list, then one wave per group walks the candidates in sequence while its lanes
//                              clear the alive bits of the later cells they own, in registers.
//
// Score threshold and top-k per image over the same cells (opt-in, this project's own rule, stated in include/skghoi.h):
//
//   skg_hoi_topk_u8          : one workgroup per image, any number of cells: a count of the candidates, a radix select of the
//                              k-th largest score key (four 8-bit passes over an LDS histogram), and a sweep in arrival order
//                              that keeps the keys above it and the first of the equal ones.
//
// Bootstrap confidence intervals of the mAP (opt-in, this project's own definition; the rule is stated in include/skghoi.h):
//
//   skg_eval_ap_boot_f64     : one wave per (class, 64 replicates) over the same sorted labels and the image id of every cell:
//                              lane = replicate, every lane walks the class in sequence with its weighted running sums in
//                              registers; '11P' or the VOC all-point area.
#include "skg_common.h"

#define EV_MAX_GT 2048            // ground-truth pairs per image the association keeps in LDS

__device__ __forceinline__ uint32_t ev_orderable(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The bid of the matching kernels for LDS atomicMax: (score, then the lower rank on ties) as one ordered 64-bit key; 0 = no
// bid.  The caller chooses the score bits: `s + 0.f` makes -0 bid like +0.
__device__ __forceinline__ unsigned long long ev_bid_key(float s, unsigned rank) {
    return ((unsigned long long)ev_orderable(s) << 32) | (0xffffffffu - rank);
}

// Inclusive scan of v over the 64 lanes of a wave, by sum or (kMax) by maximum; lane l combines lanes 0 .. l in the fixed
// order of the doubling steps.
template <bool kMax>
__device__ __forceinline__ double ev_wave_scan(double v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off, 64);
        if (lane >= off) v = kMax ? fmax(v, o) : v + o;
    }
    return v;
}

__global__ __launch_bounds__(256) void skg_eval_associate_kernel(
    const float* __restrict__ boxes_h, const float* __restrict__ boxes_o, const int64_t* __restrict__ object,
    const int32_t* __restrict__ pair_off, const int64_t* __restrict__ index, const int64_t* __restrict__ pred,
    const float* __restrict__ scores, const int32_t* __restrict__ cell_off, const int32_t* __restrict__ lut, int n_obj,
    int n_verb, const float* __restrict__ gt_h, const float* __restrict__ gt_o, const int64_t* __restrict__ gt_hoi,
    const int32_t* __restrict__ gt_off, float min_iou, int32_t* __restrict__ hoi_out, float* __restrict__ labels,
    int32_t* __restrict__ status) {
    __shared__ unsigned long long skey[EV_MAX_GT];
    const int a = blockIdx.x, tid = threadIdx.x;
    const int c0 = cell_off[a], c1 = cell_off[a + 1];
    const int g0 = gt_off[a], ng = gt_off[a + 1] - g0;
    if (ng > EV_MAX_GT) {                                    // uniform: reported, nothing written past the LDS array
        if (tid == 0) atomicMax(status, ng);
        for (int c = c0 + tid; c < c1; c += 256) { labels[c] = 0.f; hoi_out[c] = -1; }
        return;
    }
    for (int g = tid; g < ng; g += 256) skey[g] = 0ull;
    __syncthreads();
    const int p0 = pair_off[a];
    for (int c = c0 + tid; c < c1; c += 256) {
        const int64_t p = (int64_t)p0 + index[c];
        const int64_t ob = object[p], vb = pred[c];
        const int hoi = (ob >= 0 && ob < n_obj && vb >= 0 && vb < n_verb) ? lut[ob * n_verb + vb] : -1;
        hoi_out[c] = hoi;
        int match = -1;
        if (hoi >= 0) {
            const float4 dh = *reinterpret_cast<const float4*>(boxes_h + 4 * p);
            const float4 dob = *reinterpret_cast<const float4*>(boxes_o + 4 * p);
            float best = -1.f;
            for (int g = 0; g < ng; ++g) {
                if (gt_hoi[g0 + g] != hoi) continue;
                const float v = fminf(skg_iou(*reinterpret_cast<const float4*>(gt_h + 4 * (int64_t)(g0 + g)), dh),
                                      skg_iou(*reinterpret_cast<const float4*>(gt_o + 4 * (int64_t)(g0 + g)), dob));
                if (v > best) { best = v; match = g; }       // first maximum, NaN never wins
            }
            if (!(best >= min_iou)) match = -1;
        }
        if (match >= 0) atomicMax(&skey[match], ev_bid_key(scores[c], (unsigned)(c - c0)));      // the score's bits as they are
        labels[c] = match >= 0 ? __uint_as_float((unsigned)match + 1u) : 0.f;      // parked: match + 1 as raw bits
    }
    __syncthreads();
    for (int c = c0 + tid; c < c1; c += 256) {
        const unsigned m = __float_as_uint(labels[c]);
        if (m == 0u) continue;
        labels[c] = (skey[m - 1u] == ev_bid_key(scores[c], (unsigned)(c - c0))) ? 1.f : 0.f;
    }
}

extern "C" int skg_eval_associate_f32(const float* boxes_h, const float* boxes_o, const int64_t* object,
                                      const int32_t* pair_off, const int64_t* index, const int64_t* pred,
                                      const float* scores, const int32_t* cell_off, int n_images, const int32_t* lut,
                                      int n_obj, int n_verb, const float* gt_h, const float* gt_o, const int64_t* gt_hoi,
                                      const int32_t* gt_off, float min_iou, int32_t* hoi_out, float* labels,
                                      int32_t* status, void* stream) {
    if (n_images < 0 || n_obj <= 0 || n_verb <= 0) return SKG_E_ARG;
    if (n_images == 0) return 0;
    if (!boxes_h || !boxes_o || !object || !pair_off || !index || !pred || !scores || !cell_off || !lut || !gt_h || !gt_o ||
        !gt_hoi || !gt_off || !hoi_out || !labels || !status)
        return SKG_E_ARG;
    if (!skg_aligned16(boxes_h) || !skg_aligned16(boxes_o) || !skg_aligned16(gt_h) || !skg_aligned16(gt_o))
        return SKG_E_ALIGN;
    hipLaunchKernelGGL(skg_eval_associate_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, boxes_h, boxes_o,
                       object, pair_off, index, pred, scores, cell_off, lut, n_obj, n_verb, gt_h, gt_o, gt_hoi, gt_off,
                       min_iou, hoi_out, labels, status);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ Known Object setting
// HICO-DET's second setting (Chao et al., WACV 2018; the official evaluation is outside the reference tree, the published
// rule is restated in include/skghoi.h -- parity unpinned at that boundary): a cell of class h counts only in the images
// whose ground truth holds the object category of h, through whichever interaction class.  One workgroup per image: the
// object categories of the image's ground-truth pairs as a bit mask in LDS (nothing per pair: no cap on the pairs), then one
// flag per cell.
__global__ __launch_bounds__(256) void skg_eval_known_object_kernel(
    const int32_t* __restrict__ hoi, const int32_t* __restrict__ cell_off, const int32_t* __restrict__ hoi_object, int n_hoi,
    int n_obj, const int64_t* __restrict__ gt_hoi, const int32_t* __restrict__ gt_off, uint8_t* __restrict__ keep) {
    __shared__ unsigned smask[SKG_EVAL_MAX_OBJECTS / 32];
    const int a = blockIdx.x, tid = threadIdx.x;
    for (int w = tid; w < (n_obj + 31) / 32; w += 256) smask[w] = 0u;      // n_obj <= SKG_EVAL_MAX_OBJECTS: checked by the entry
    __syncthreads();
    const int g1 = gt_off[a + 1];
    for (int g = gt_off[a] + tid; g < g1; g += 256) {
        const int64_t h = gt_hoi[g];
        if (h < 0 || h >= n_hoi) continue;                   // the -1 padding row, ids outside the classes
        const int o = hoi_object[h];
        if (o >= 0 && o < n_obj) atomicOr(&smask[o >> 5], 1u << (o & 31));
    }
    __syncthreads();
    const int c1 = cell_off[a + 1];
    for (int c = cell_off[a] + tid; c < c1; c += 256) {
        const int h = hoi[c];
        const int o = (h >= 0 && h < n_hoi) ? hoi_object[h] : -1;
        keep[c] = (o >= 0 && o < n_obj) ? (uint8_t)((smask[o >> 5] >> (o & 31)) & 1u) : (uint8_t)0;
    }
}

extern "C" int skg_eval_known_object_u8(const int32_t* hoi, const int32_t* cell_off, int n_images, const int32_t* hoi_object,
                                        int n_hoi, int n_obj, const int64_t* gt_hoi, const int32_t* gt_off, uint8_t* keep,
                                        void* stream) {
    if (n_images < 0 || n_hoi <= 0 || n_obj <= 0) return SKG_E_ARG;
    if (n_obj > SKG_EVAL_MAX_OBJECTS) return SKG_E_LIMIT;
    if (n_images == 0) return 0;
    if (!hoi || !cell_off || !hoi_object || !gt_hoi || !gt_off || !keep) return SKG_E_ARG;
    hipLaunchKernelGGL(skg_eval_known_object_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, hoi, cell_off,
                       hoi_object, n_hoi, n_obj, gt_hoi, gt_off, keep);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ error breakdown
// Where the Default mAP is lost inside the head: one category per cell (tp, duplicate, verb, object, human, background) and
// one status per ground-truth pair (hit, shadowed, unscored, unpaired).  Not part of the reference: this project's own
// definition in the spirit of TIDE-style detection diagnostics, the rule is stated in include/skghoi.h -- parity unpinned,
// there is nothing to be on a par with.  Launched behind the association on its hoi_out and final labels.  One workgroup
// per image: one flag word per ground-truth pair in LDS (EV_MAX_GT x 4 bytes = 8 KB; bit 0 = the match of a true positive,
// bit 1 = covered by a cell of its class).  Lanes stride over the cells, one pass over the ground truth each collecting the
// five predicates (a true positive repeats the association's arg-max and flags its match); after a barrier lanes stride
// over the ground-truth pairs and, for the ones no cell of their class covered, walk the image's output pairs.  Every
// barrier is reached by all lanes (the early return of an image above the cap is uniform), every output byte is written once.
#define EV_ERR_HIT 1u
#define EV_ERR_SCORED 2u

__global__ __launch_bounds__(256) void skg_eval_hoi_errors_kernel(
    const float* __restrict__ boxes_h, const float* __restrict__ boxes_o, const int32_t* __restrict__ pair_off,
    const int64_t* __restrict__ index, const int32_t* __restrict__ hoi, const float* __restrict__ labels,
    const int32_t* __restrict__ cell_off, const int32_t* __restrict__ hoi_object, int n_hoi, const float* __restrict__ gt_h,
    const float* __restrict__ gt_o, const int64_t* __restrict__ gt_hoi, const int32_t* __restrict__ gt_off, float min_iou,
    uint8_t* __restrict__ category, uint8_t* __restrict__ gt_status) {
    __shared__ unsigned sflag[EV_MAX_GT];
    const int a = blockIdx.x, tid = threadIdx.x;
    const int c0 = cell_off[a], c1 = cell_off[a + 1];
    const int g0 = gt_off[a], ng = gt_off[a + 1] - g0;
    if (ng > EV_MAX_GT) {                                    // uniform: the association refused the image, summary() raises
        for (int c = c0 + tid; c < c1; c += 256) category[c] = (uint8_t)255;
        for (int g = tid; g < ng; g += 256) gt_status[g0 + g] = (uint8_t)255;
        return;
    }
    for (int g = tid; g < ng; g += 256) sflag[g] = 0u;
    __syncthreads();
    const int p0 = pair_off[a], p1 = pair_off[a + 1];
    for (int c = c0 + tid; c < c1; c += 256) {
        const int h = hoi[c];
        if (h < 0 || h >= n_hoi) { category[c] = (uint8_t)255; continue; }
        const int oc = hoi_object[h];
        const int64_t p = (int64_t)p0 + index[c];
        const float4 dh = *reinterpret_cast<const float4*>(boxes_h + 4 * p);
        const float4 dob = *reinterpret_cast<const float4*>(boxes_o + 4 * p);
        bool dup = false, verb = false, obj = false, hum = false;
        float best = -1.f;
        int match = -1;
        for (int g = 0; g < ng; ++g) {
            const int64_t t = gt_hoi[g0 + g];
            if (t < 0 || t >= n_hoi) continue;               // invalid pairs take no part
            const bool same = t == (int64_t)h;
            if (!same) {
                const int ot = hoi_object[t];
                if (ot < 0 || ot != oc) continue;            // another object category: no predicate reads this pair
            }
            const float ih = skg_iou(*reinterpret_cast<const float4*>(gt_h + 4 * (int64_t)(g0 + g)), dh);
            const float io = skg_iou(*reinterpret_cast<const float4*>(gt_o + 4 * (int64_t)(g0 + g)), dob);
            const bool ch = ih >= min_iou, co = io >= min_iou;       // NaN: false
            if (same) {
                if (ch && co) { dup = true; atomicOr(&sflag[g], EV_ERR_SCORED); }
                obj |= ch; hum |= co;
                const float v = fminf(ih, io);
                if (v > best) { best = v; match = g; }       // the association's arg-max: first maximum, NaN never wins
            } else if (ch && co) {
                verb = true;
            }
        }
        if (labels[c] == 1.f) {
            if (match >= 0) atomicOr(&sflag[match], EV_ERR_HIT);
            category[c] = (uint8_t)0;
        } else {
            category[c] = (uint8_t)(dup ? 1 : verb ? 2 : obj ? 3 : hum ? 4 : 5);
        }
    }
    __syncthreads();
    for (int g = tid; g < ng; g += 256) {
        const int64_t t = gt_hoi[g0 + g];
        if (t < 0 || t >= n_hoi) { gt_status[g0 + g] = (uint8_t)255; continue; }
        const unsigned f = sflag[g];
        int st = (f & EV_ERR_HIT) ? 0 : (f & EV_ERR_SCORED) ? 1 : 3;
        if (st == 3) {
            const float4 gh = *reinterpret_cast<const float4*>(gt_h + 4 * (int64_t)(g0 + g));
            const float4 go = *reinterpret_cast<const float4*>(gt_o + 4 * (int64_t)(g0 + g));
            for (int p = p0; p < p1; ++p) {
                if (skg_iou(gh, *reinterpret_cast<const float4*>(boxes_h + 4 * (int64_t)p)) >= min_iou &&
                    skg_iou(go, *reinterpret_cast<const float4*>(boxes_o + 4 * (int64_t)p)) >= min_iou) {
                    st = 2;
                    break;
                }
            }
        }
        gt_status[g0 + g] = (uint8_t)st;
    }
}

extern "C" int skg_eval_hoi_errors_u8(const float* boxes_h, const float* boxes_o, const int32_t* pair_off, const int64_t* index,
                                      const int32_t* hoi, const float* labels, const int32_t* cell_off, int n_images,
                                      const int32_t* hoi_object, int n_hoi, const float* gt_h, const float* gt_o,
                                      const int64_t* gt_hoi, const int32_t* gt_off, float min_iou, uint8_t* category,
                                      uint8_t* gt_status, void* stream) {
    if (n_images < 0 || n_hoi <= 0) return SKG_E_ARG;
    if (n_images == 0) return 0;
    if (!boxes_h || !boxes_o || !pair_off || !index || !hoi || !labels || !cell_off || !hoi_object || !gt_h || !gt_o ||
        !gt_hoi || !gt_off || !category || !gt_status)
        return SKG_E_ARG;
    if (!skg_aligned16(boxes_h) || !skg_aligned16(boxes_o) || !skg_aligned16(gt_h) || !skg_aligned16(gt_o))
        return SKG_E_ALIGN;
    hipLaunchKernelGGL(skg_eval_hoi_errors_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, boxes_h, boxes_o,
                       pair_off, index, hoi, labels, cell_off, hoi_object, n_hoi, gt_h, gt_o, gt_hoi, gt_off, min_iou,
                       category, gt_status);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ 11-point AP
// labels_sorted: the 0/1 labels of all detections, sorted by class (ascending) and inside a class by score (descending,
// ties in arrival order); class_off[c .. c+1] = the class's range.  ap[c] = (1/11) sum_k max{prec_i : rec_i >= thr[k]},
// prec_i = tp_i / (i + 1), rec_i = tp_i / num_gt[c]; 0 for a class without ground truth or detections.
__global__ __launch_bounds__(256) void skg_eval_ap11_kernel(const float* __restrict__ labels_sorted,
                                                            const int64_t* __restrict__ class_off,
                                                            const int64_t* __restrict__ num_gt,
                                                            const double* __restrict__ thr, double* __restrict__ ap) {
    __shared__ double swave[4];
    __shared__ double sbase;
    __shared__ double smax[4][11];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t s0 = class_off[c], s1 = class_off[c + 1];
    const double ng = (double)num_gt[c];
    if (ng <= 0.0 || s1 <= s0) { if (tid == 0) ap[c] = 0.0; return; }
    double t[11], best[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) { t[k] = thr[k]; best[k] = 0.0; }
    if (tid == 0) sbase = 0.0;
    __syncthreads();
    for (int64_t i0 = s0; i0 < s1; i0 += 256) {
        const int64_t i = i0 + tid;
        const double y = i < s1 ? (double)labels_sorted[i] : 0.0;
        const double inc = ev_wave_scan<false>(y, lane);     // per wave; the waves before it are added below
        if (lane == 63) swave[wv] = inc;
        __syncthreads();
        double tp = sbase + inc;
        for (int w = 0; w < wv; ++w) tp += swave[w];
        if (i < s1) {
            const double prec = tp / (double)(i - s0 + 1), rec = tp / ng;
#pragma unroll
            for (int k = 0; k < 11; ++k)
                if (rec >= t[k] && prec > best[k]) best[k] = prec;
        }
        __syncthreads();
        if (tid == 0) sbase += (swave[0] + swave[1]) + (swave[2] + swave[3]);
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        double v = best[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
        if (lane == 0) smax[wv][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < 11; ++k) s += fmax(fmax(smax[0][k], smax[1][k]), fmax(smax[2][k], smax[3][k])) / 11.0;
        ap[c] = s;
    }
}

extern "C" int skg_eval_ap11_f64(const float* labels_sorted, const int64_t* class_off, const int64_t* num_gt, int n_classes,
                                 const double* thresholds11, double* ap, void* stream) {
    if (n_classes < 0) return SKG_E_ARG;
    if (n_classes == 0) return 0;
    if (!class_off || !num_gt || !thresholds11 || !ap) return SKG_E_ARG;
    hipLaunchKernelGGL(skg_eval_ap11_kernel, dim3(n_classes), dim3(256), 0, (hipStream_t)stream, labels_sorted, class_off,
                       num_gt, thresholds11, ap);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ V-COCO role matching
__device__ __forceinline__ float ev_iou_px(const float4 a, const float4 b) {     // the toolkit's get_overlap: pixel indices
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x) + 1.f, 0.f), h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y) + 1.f, 0.f);
    const float inter = w * h;
    const float aa = (a.z - a.x + 1.f) * (a.w - a.y + 1.f), ab = (b.z - b.x + 1.f) * (b.w - b.y + 1.f);
    return inter / (aa + ab - inter);                        // a NaN coordinate makes its area, and so the IoU, NaN
}

__global__ __launch_bounds__(256) void skg_eval_vcoco_match_kernel(
    const float* __restrict__ boxes_h, const float* __restrict__ boxes_o, const int32_t* __restrict__ pair_off,
    const int64_t* __restrict__ index, const int64_t* __restrict__ pred, const float* __restrict__ scores,
    const int32_t* __restrict__ cell_off, const int32_t* __restrict__ class_ar, const float* __restrict__ persons,
    const int8_t* __restrict__ actions, const float* __restrict__ role_boxes, const int32_t* __restrict__ gt_off, float thr,
    int8_t* __restrict__ labels_s1, int8_t* __restrict__ labels_s2, int32_t* __restrict__ status) {
    __shared__ unsigned long long skey[2][SKG_VCOCO_MAX_PERSONS];
    __shared__ float4 sper[SKG_VCOCO_MAX_PERSONS];
    __shared__ int sact[SKG_VCOCO_MAX_PERSONS];              // actions[j, aid]; -2 for an ignored person
    const int a = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int c0 = cell_off[a], c1 = cell_off[a + 1];
    const int g0 = gt_off[a], ng = gt_off[a + 1] - g0;
    const int p0 = pair_off[a], np = pair_off[a + 1] - p0;
    const int aid = class_ar[2 * k], rid = class_ar[2 * k + 1];
    const bool known = aid >= 0 && aid < SKG_VCOCO_ACTIONS && rid >= 0 && rid < 2;
    if (ng > SKG_VCOCO_MAX_PERSONS || !known) {              // uniform: reported, nothing written past the LDS arrays
        if (tid == 0 && k == 0 && ng > SKG_VCOCO_MAX_PERSONS) atomicMax(status, ng);
        for (int c = c0 + tid; c < c1; c += 256)
            if (pred[c] == k) { labels_s1[c] = 0; labels_s2[c] = 0; }
        return;
    }
    for (int g = tid; g < ng; g += 256) {
        skey[0][g] = 0ull; skey[1][g] = 0ull;
        sper[g] = *reinterpret_cast<const float4*>(persons + 4 * (int64_t)(g0 + g));
        const int8_t* act = actions + (int64_t)(g0 + g) * SKG_VCOCO_ACTIONS;
        bool ignored = false;
        for (int t = 0; t < SKG_VCOCO_ACTIONS; ++t) ignored |= act[t] == -1;
        sact[g] = ignored ? -2 : (int)act[aid];
    }
    __syncthreads();
    for (int c = c0 + tid; c < c1; c += 256) {
        if (pred[c] != k) continue;
        const float s = scores[c];
        const int64_t li = index[c];
        int8_t o1 = 0, o2 = 0;                               // parked for the second pass: o1 = jmax, o2 = candidate bits
        if (s != s) { o1 = -1; o2 = -1; }                    // NaN score: dropped
        else if (ng > 0 && (uint64_t)li < (uint64_t)np) {
            const float4 dh = *reinterpret_cast<const float4*>(boxes_h + 4 * ((int64_t)p0 + li));
            float best = -1.f; int jmax = 0;
            for (int g = 0; g < ng; ++g) {
                const float v = ev_iou_px(sper[g], dh);
                if (v > best) { best = v; jmax = g; }        // first maximum, NaN never wins
            }
            const int act = sact[jmax];
            if (act == -2) { o1 = -1; o2 = -1; }             // the best person is not annotated: dropped
            else if (act == 1 && best >= thr) {
                const float4 dob = *reinterpret_cast<const float4*>(boxes_o + 4 * ((int64_t)p0 + li));
                const float4 rb = *reinterpret_cast<const float4*>(
                    role_boxes + 4 * ((((int64_t)(g0 + jmax)) * SKG_VCOCO_ACTIONS + aid) * 2 + rid));
                float ov1, ov2;
                if (rb.x == -1.f && rb.y == -1.f && rb.z == -1.f && rb.w == -1.f) {
                    const bool empty = (dob.x == 0.f && dob.y == 0.f && dob.z == 0.f && dob.w == 0.f) ||
                                       (dob.x != dob.x && dob.y != dob.y && dob.z != dob.z && dob.w != dob.w);
                    ov1 = empty ? 1.f : 0.f; ov2 = 1.f;
                } else {
                    ov1 = ov2 = ev_iou_px(rb, dob);
                }
                const int bits = (ov1 >= thr ? 1 : 0) | (ov2 >= thr ? 2 : 0);
                if (bits) {
                    const unsigned long long key = ev_bid_key(s + 0.f, (unsigned)(c - c0));      // s + 0: -0 bids like +0
                    if (bits & 1) atomicMax(&skey[0][jmax], key);
                    if (bits & 2) atomicMax(&skey[1][jmax], key);
                    o1 = (int8_t)(uint8_t)jmax; o2 = (int8_t)bits;
                }
            }
        }
        labels_s1[c] = o1; labels_s2[c] = o2;
    }
    __syncthreads();
    for (int c = c0 + tid; c < c1; c += 256) {               // the same lane reads back what it parked
        if (pred[c] != k) continue;
        const int bits = labels_s2[c];
        if (bits <= 0) continue;                             // final already: 0 or -1 in both
        const int jmax = (int)(uint8_t)labels_s1[c];
        const unsigned long long key = ev_bid_key(scores[c] + 0.f, (unsigned)(c - c0));
        labels_s1[c] = ((bits & 1) && skey[0][jmax] == key) ? 1 : 0;
        labels_s2[c] = ((bits & 2) && skey[1][jmax] == key) ? 1 : 0;
    }
}

extern "C" int skg_eval_vcoco_match_f32(const float* boxes_h, const float* boxes_o, const int32_t* pair_off,
                                        const int64_t* index, const int64_t* pred, const float* scores,
                                        const int32_t* cell_off, int n_images, const int32_t* class_ar, int n_classes,
                                        const float* persons, const int8_t* actions, const float* role_boxes,
                                        const int32_t* gt_off, float thr, int8_t* labels_s1, int8_t* labels_s2,
                                        int32_t* status, void* stream) {
    if (n_images < 0 || n_classes <= 0 || n_classes > SKG_VCOCO_MAX_CLASSES) return SKG_E_ARG;
    if (!boxes_h || !boxes_o || !pair_off || !index || !pred || !scores || !cell_off || !class_ar || !persons || !actions ||
        !role_boxes || !gt_off || !labels_s1 || !labels_s2 || !status)
        return SKG_E_ARG;
    if (!skg_aligned16(boxes_h) || !skg_aligned16(boxes_o) || !skg_aligned16(persons) || !skg_aligned16(role_boxes))
        return SKG_E_ALIGN;
    if (n_images == 0) return 0;
    hipLaunchKernelGGL(skg_eval_vcoco_match_kernel, dim3(n_images, n_classes), dim3(256), 0, (hipStream_t)stream, boxes_h,
                       boxes_o, pair_off, index, pred, scores, cell_off, class_ar, persons, actions, role_boxes, gt_off, thr,
                       labels_s1, labels_s2, status);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ VOC all-point AP
// Same inputs as skg_eval_ap11_f64.  With tp_i the running sum of the labels and prec_i = tp_i / (i + 1),
// ap[c] = (1 / num_gt[c]) sum_i label_i * max_{j >= i} prec_j.  The class is walked from its end in tiles of 256 with lane
// t on position end - 1 - t, so that an inclusive scan over the lanes is a suffix scan over the positions.
__global__ __launch_bounds__(256) void skg_eval_ap_voc_kernel(const float* __restrict__ labels_sorted,
                                                              const int64_t* __restrict__ class_off,
                                                              const int64_t* __restrict__ num_gt, double* __restrict__ ap) {
    __shared__ double swsum[4], swmax[4], sred[4];
    __shared__ double sbase_sum, sbase_max;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t s0 = class_off[c], s1 = class_off[c + 1];
    const double ng = (double)num_gt[c];
    if (ng <= 0.0 || s1 <= s0) { if (tid == 0) ap[c] = 0.0; return; }
    double total = 0.0;                                      // the class's true positives
    for (int64_t i = s0 + tid; i < s1; i += 256) total += (double)labels_sorted[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
    if (lane == 0) sred[wv] = total;
    if (tid == 0) { sbase_sum = 0.0; sbase_max = 0.0; }
    __syncthreads();
    total = (sred[0] + sred[1]) + (sred[2] + sred[3]);
    double acc = 0.0;
    for (int64_t e = s1; e > s0; e -= 256) {
        const int64_t i = e - 1 - tid;
        const bool valid = i >= s0;
        const double y = valid ? (double)labels_sorted[i] : 0.0;
        const double inc = ev_wave_scan<false>(y, lane);     // labels at positions >= i of this wave's part of the tile
        if (lane == 63) swsum[wv] = inc;
        __syncthreads();
        double behind = sbase_sum + (inc - y);               // labels at positions > i of the class
        for (int w = 0; w < wv; ++w) behind += swsum[w];
        // prec_i, then its suffix maximum
        double m = ev_wave_scan<true>(valid ? (total - behind) / (double)(i - s0 + 1) : 0.0, lane);
        if (lane == 63) swmax[wv] = m;
        __syncthreads();
        m = fmax(m, sbase_max);
        for (int w = 0; w < wv; ++w) m = fmax(m, swmax[w]);
        acc += y * m;
        __syncthreads();
        if (tid == 0) {
            sbase_sum += (swsum[0] + swsum[1]) + (swsum[2] + swsum[3]);
            sbase_max = fmax(fmax(sbase_max, fmax(swmax[0], swmax[1])), fmax(swmax[2], swmax[3]));
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) sred[wv] = acc;
    __syncthreads();
    if (tid == 0) ap[c] = ((sred[0] + sred[1]) + (sred[2] + sred[3])) / ng;
}

extern "C" int skg_eval_ap_voc_f64(const float* labels_sorted, const int64_t* class_off, const int64_t* num_gt, int n_classes,
                                   double* ap, void* stream) {
    if (n_classes < 0) return SKG_E_ARG;
    if (n_classes == 0) return 0;
    if (!class_off || !num_gt || !ap) return SKG_E_ARG;
    hipLaunchKernelGGL(skg_eval_ap_voc_kernel, dim3(n_classes), dim3(256), 0, (hipStream_t)stream, labels_sorted, class_off,
                       num_gt, ap);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ object detections
// The rule is stated in include/skghoi.h (skg_eval_det_match_f32).  LDS of the match kernel: 1024 boxes (16 KB), their classes
// as int64 (8 KB), the bid keys (8 KB), the suppression bytes (1 KB): 33 KB static, under the 64 KB a workgroup may declare.
#define EVD_CHUNK 256             // detections per LDS chunk of the pair-coverage kernel

// one ground-truth box on the coordinate trick's offset: batched_nms's `boxes + (idxs.to(boxes) * (max_coord + 1))[:, None]`
__device__ __forceinline__ float4 evd_shifted(const float4 b, int64_t cls, float unit) {
    const float off = (float)cls * unit;
    return make_float4(b.x + off, b.y + off, b.z + off, b.w + off);
}

__global__ __launch_bounds__(256) void skg_eval_det_match_kernel(
    const float* __restrict__ det_boxes, const float* __restrict__ det_scores, const int64_t* __restrict__ det_labels,
    const int32_t* __restrict__ det_off, const float* __restrict__ gt_h, const float* __restrict__ gt_o,
    const int64_t* __restrict__ gt_object, const int32_t* __restrict__ gt_off, int human_idx, int num_classes, float min_iou,
    float nms_thresh, int8_t* __restrict__ labels, int32_t* __restrict__ matched_gt, uint8_t* __restrict__ gt_keep,
    unsigned long long* __restrict__ num_gt, int32_t* __restrict__ status) {
    __shared__ float4 sbox[SKG_EVAL_DET_MAX_GT];             // cat(boxes_h, boxes_o) of the image, unshifted
    __shared__ int64_t scls[SKG_EVAL_DET_MAX_GT];
    __shared__ unsigned long long skey[SKG_EVAL_DET_MAX_GT];
    __shared__ unsigned char ssup[SKG_EVAL_DET_MAX_GT];
    __shared__ float sred[4];
    __shared__ int snan;
    const int a = blockIdx.x, tid = threadIdx.x;
    const int d0 = det_off[a], d1 = det_off[a + 1];
    const int g0 = gt_off[a];
    const int G = max(gt_off[a + 1] - g0, 0);
    if (G > SKG_EVAL_DET_MAX_GT / 2) {                       // uniform, ahead of every barrier: reported, nothing staged
        if (tid == 0) atomicMax(status, G > 0x3fffffff ? 0x7fffffff : 2 * G);
        for (int d = d0 + tid; d < d1; d += 256) { labels[d] = 0; matched_gt[d] = -1; }
        for (int64_t j = tid; j < 2 * (int64_t)G; j += 256) gt_keep[2 * (int64_t)g0 + j] = 0;
        return;
    }
    const int nb = 2 * G;

    // ---- phase 1: the ground-truth box set.  Staging, max_coord (NaN propagates like Tensor.max()), greedy NMS in index order
    if (tid == 0) snan = 0;
    float lmax = -INFINITY;
    bool lnan = false;
    for (int j = tid; j < nb; j += 256) {
        const bool hum = j < G;
        const int64_t g = (int64_t)g0 + (hum ? j : j - G);
        const float4 b = *reinterpret_cast<const float4*>((hum ? gt_h : gt_o) + 4 * g);
        sbox[j] = b; scls[j] = hum ? (int64_t)human_idx : gt_object[g]; skey[j] = 0ull; ssup[j] = 0;
        lmax = fmaxf(lmax, fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
        lnan |= (b.x != b.x) | (b.y != b.y) | (b.z != b.z) | (b.w != b.w);
    }
    lmax = skg_wave_max(lmax);
    if ((tid & 63) == 0) sred[tid >> 6] = lmax;
    __syncthreads();
    if (lnan) snan = 1;                                      // (every writer stores the same value)
    __syncthreads();
    float max_coord = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
    // one NaN coordinate makes every offset, shifted box, area and IoU NaN: `IoU > thr` never holds, nothing is suppressed
    if (snan) max_coord = __uint_as_float(0x7fc00000u);
    const float unit = max_coord + 1.0f;
    for (int i = 0; i < nb; ++i) {                           // sequential over the candidates, the lanes suppress in parallel
        if (!ssup[i]) {                                      // uniform (LDS broadcast; final since the previous barrier)
            const float4 bi = evd_shifted(sbox[i], scls[i], unit);
            const float ai = (bi.z - bi.x) * (bi.w - bi.y);
            for (int j = i + 1 + tid; j < nb; j += 256) {
                if (ssup[j]) continue;
                const float4 bj = evd_shifted(sbox[j], scls[j], unit);
                const float aj = (bj.z - bj.x) * (bj.w - bj.y);
                const float xx1 = fmaxf(bi.x, bj.x), yy1 = fmaxf(bi.y, bj.y);
                const float xx2 = fminf(bi.z, bj.z), yy2 = fminf(bi.w, bj.w);
                const float w = fmaxf(xx2 - xx1, 0.f), h = fmaxf(yy2 - yy1, 0.f);
                const float inter = w * h;
                const float ovr = inter / (ai + aj - inter);
                if (ovr > nms_thresh) ssup[j] = 1;
            }
        }
        __syncthreads();
    }
    int bad = 0;
    for (int j = tid; j < nb; j += 256) {
        const bool kept = ssup[j] == 0;
        gt_keep[2 * (int64_t)g0 + j] = kept ? 1 : 0;
        if (kept) {
            const int64_t c = scls[j];
            if (c >= 0 && c < num_classes) atomicAdd(&num_gt[c], 1ull);      // integer: order-independent
            else ++bad;
        }
    }
    if (bad) atomicAdd(status + 1, bad);

    // ---- phase 2: every detection finds the kept box of its class of largest plain IoU and bids for it
    for (int d = d0 + tid; d < d1; d += 256) {
        const float s = det_scores[d];
        const int64_t c = det_labels[d];
        int match = -1;
        if (s == s && c >= 0 && c < num_classes) {           // a NaN score never bids
            const float4 db = *reinterpret_cast<const float4*>(det_boxes + 4 * (int64_t)d);
            float best = -1.f;
            for (int j = 0; j < nb; ++j) {
                if (ssup[j] || scls[j] != c) continue;
                const float v = skg_iou(sbox[j], db);
                if (v > best) { best = v; match = j; }       // first maximum, NaN never wins
            }
            if (!(best >= min_iou)) match = -1;
            if (match >= 0) atomicMax(&skey[match], ev_bid_key(s + 0.f, (unsigned)(d - d0)));      // s + 0: -0 bids like +0
        }
        matched_gt[d] = match;                               // final; the same lane reads it back behind the barrier
    }
    __syncthreads();
    for (int d = d0 + tid; d < d1; d += 256) {
        const float s = det_scores[d];
        int8_t lab = 0;
        if (s != s) lab = -1;                                // dropped
        else {
            const int m = matched_gt[d];
            if (m >= 0) lab = skey[m] == ev_bid_key(s + 0.f, (unsigned)(d - d0)) ? 1 : 0;
        }
        labels[d] = lab;
    }
}

extern "C" int skg_eval_det_match_f32(const float* det_boxes, const float* det_scores, const int64_t* det_labels,
                                      const int32_t* det_off, int n_images, const float* gt_h, const float* gt_o,
                                      const int64_t* gt_object, const int32_t* gt_off, int human_idx, int num_classes,
                                      float min_iou, float nms_thresh, int8_t* labels, int32_t* matched_gt, uint8_t* gt_keep,
                                      int64_t* num_gt, int32_t* status, void* stream) {
    if (n_images < 0 || num_classes <= 0 || human_idx < 0 || human_idx >= num_classes) return SKG_E_ARG;
    if (!det_boxes || !det_scores || !det_labels || !det_off || !gt_h || !gt_o || !gt_object || !gt_off || !labels ||
        !matched_gt || !gt_keep || !num_gt || !status)
        return SKG_E_ARG;
    if (!skg_aligned16(det_boxes) || !skg_aligned16(gt_h) || !skg_aligned16(gt_o)) return SKG_E_ALIGN;
    if (n_images == 0) return 0;
    hipLaunchKernelGGL(skg_eval_det_match_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, det_boxes, det_scores,
                       det_labels, det_off, gt_h, gt_o, gt_object, gt_off, human_idx, num_classes, min_iou, nms_thresh, labels,
                       matched_gt, gt_keep, reinterpret_cast<unsigned long long*>(num_gt), status);
    return skg_launch_status();
}

// Pair coverage.  One lane per ground-truth pair (tiles of 256 pairs), the image's detections through LDS in chunks of
// EVD_CHUNK: every loop bound is uniform over the workgroup, so that all 256 lanes reach every barrier.  Dropped detections
// (labels_in < 0: the match kernel's NaN scores) are staged with a flag and skipped.
__global__ __launch_bounds__(256) void skg_eval_pair_cover_kernel(
    const float* __restrict__ det_boxes, const int64_t* __restrict__ det_labels, const int8_t* __restrict__ labels_in,
    const int32_t* __restrict__ det_off, const float* __restrict__ gt_h, const float* __restrict__ gt_o,
    const int64_t* __restrict__ gt_object, const int32_t* __restrict__ gt_off, int human_idx, float min_iou,
    uint8_t* __restrict__ covered) {
    __shared__ float4 sdb[EVD_CHUNK];
    __shared__ int64_t sdc[EVD_CHUNK];
    __shared__ unsigned char sdrop[EVD_CHUNK];
    const int a = blockIdx.x, tid = threadIdx.x;
    const int d0 = det_off[a], nd = max(det_off[a + 1] - d0, 0);
    const int g0 = gt_off[a], G = max(gt_off[a + 1] - g0, 0);
    for (int gb = 0; gb < G; gb += 256) {                    // uniform
        const bool valid = gb + tid < G;
        const int64_t g = (int64_t)g0 + gb + tid;
        float4 bh = make_float4(0.f, 0.f, 0.f, 0.f), bo = bh;
        int64_t ob = 0;
        if (valid) {
            bh = *reinterpret_cast<const float4*>(gt_h + 4 * g);
            bo = *reinterpret_cast<const float4*>(gt_o + 4 * g);
            ob = gt_object[g];
        }
        int nh = 0, no = 0, fh = -1, fo = -1;                // qualifying detections per side and the first index of each
        for (int k0 = 0; k0 < nd; k0 += EVD_CHUNK) {         // uniform
            const int nk = min(EVD_CHUNK, nd - k0);
            __syncthreads();                                 // the previous chunk is read
            for (int k = tid; k < nk; k += 256) {
                const int64_t d = (int64_t)d0 + k0 + k;
                sdb[k] = *reinterpret_cast<const float4*>(det_boxes + 4 * d);
                sdc[k] = det_labels[d];
                sdrop[k] = labels_in[d] < 0 ? 1 : 0;
            }
            __syncthreads();
            if (valid) {
                for (int k = 0; k < nk; ++k) {
                    if (sdrop[k]) continue;
                    const int64_t c = sdc[k];
                    if (c == (int64_t)human_idx && skg_iou(bh, sdb[k]) >= min_iou) { if (nh++ == 0) fh = k0 + k; }
                    if (c == ob && skg_iou(bo, sdb[k]) >= min_iou) { if (no++ == 0) fo = k0 + k; }
                }
            }
        }
        if (valid) covered[g] = (nh >= 1 && no >= 1 && !(nh == 1 && no == 1 && fh == fo)) ? 1 : 0;
    }
}

extern "C" int skg_eval_pair_cover_u8(const float* det_boxes, const int64_t* det_labels, const int8_t* labels_in,
                                      const int32_t* det_off, int n_images, const float* gt_h, const float* gt_o,
                                      const int64_t* gt_object, const int32_t* gt_off, int human_idx, float min_iou,
                                      uint8_t* covered, void* stream) {
    if (n_images < 0) return SKG_E_ARG;
    if (!det_boxes || !det_labels || !labels_in || !det_off || !gt_h || !gt_o || !gt_object || !gt_off || !covered)
        return SKG_E_ARG;
    if (!skg_aligned16(det_boxes) || !skg_aligned16(gt_h) || !skg_aligned16(gt_o)) return SKG_E_ALIGN;
    if (n_images == 0) return 0;
    hipLaunchKernelGGL(skg_eval_pair_cover_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, det_boxes, det_labels,
                       labels_in, det_off, gt_h, gt_o, gt_object, gt_off, human_idx, min_iou, covered);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ pair NMS
// Suppression of duplicate (human, object, class) triplets among the head's scored cells, per image -- the remedy the error
// breakdown's `duplicate` category points at.  Not part of the reference: restated from the published idea (PPDM's PNMS; the
// triplet_nms_filter of QPIC / CDN without the fractional exponents) -- parity unpinned; the rule is stated in
// include/skghoi.h (skg_hoi_pair_nms_u8).  `order` puts the batch's cells in (image, group, score descending, arrival) order.
// One workgroup per image.  Phase 1: lanes stride over the image's sorted positions in tiles of 256 and compact the positions
// where the group changes into an LDS list (wave ballots + four wave counts; two barriers per tile, every loop bound uniform);
// every order entry and every pair index is range-checked here, ahead of any write.  An image above a cap, or a malformed one,
// leaves through a uniform early path (keep = 1 everywhere, reported through status).  Phase 2 has no barrier: the four waves
// take the groups round-robin; lane l owns the group's cells l, l + 64, ... with one alive bit and one pair index each in
// registers (PN_SLOTS of them), the wave walks the candidates in sequence, reads the candidate's alive bit from its owner by
// a shuffle (wave-uniform: all 64 lanes reach every shuffle) and the owners clear the bits of their later cells.  Nothing
// passes between lanes through memory, so no wave-synchronous assumption is made.  LDS: 16 KB + a few words.
#define PN_SLOTS (SKG_PAIR_NMS_MAX_GROUP_CELLS / 64)

// sorted position s of image [c0, c1) with pairs [p0, p0 + np) -> its cell, global pair index and group key; false = malformed
__device__ __forceinline__ bool pn_cell(const int64_t* __restrict__ order, const int64_t* __restrict__ index,
                                        const int64_t* __restrict__ object, const int64_t* __restrict__ pred, int s, int c0,
                                        int c1, int p0, int np, int64_t& ob, int64_t& pr) {
    const int64_t c = order[s];
    if (c < c0 || c >= c1) return false;
    const int64_t li = index[c];
    if ((uint64_t)li >= (uint64_t)np) return false;
    ob = object[(int64_t)p0 + li]; pr = pred[c];
    return true;
}

__global__ __launch_bounds__(256) void skg_hoi_pair_nms_kernel(
    const float* __restrict__ boxes_h, const float* __restrict__ boxes_o, const int64_t* __restrict__ object,
    const int32_t* __restrict__ pair_off, const int64_t* __restrict__ index, const int64_t* __restrict__ pred,
    const float* __restrict__ scores, const int32_t* __restrict__ cell_off, const int64_t* __restrict__ order, int measure,
    float thresh, uint8_t* __restrict__ keep, int32_t* __restrict__ status) {
    __shared__ int sstart[SKG_PAIR_NMS_MAX_GROUPS + 1];      // sorted positions where a group starts, then the image's end
    __shared__ int swave[4];
    __shared__ int sbad, slong;
    const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c0 = cell_off[a], c1 = cell_off[a + 1];
    const int p0 = pair_off[a], np = pair_off[a + 1] - p0;
    if (c1 <= c0) return;                                    // uniform: an image without cells
    if (tid == 0) { sbad = 0; slong = 0; }
    __syncthreads();

    // ---- phase 1: the group starts, in order
    int ng = 0;                                              // the same in every lane
    for (int s0 = c0; s0 < c1; s0 += 256) {                  // uniform
        const int s = s0 + tid;
        bool start = false;
        if (s < c1) {
            int64_t ob = 0, pr = 0, ob1 = 0, pr1 = 0;
            bool ok = pn_cell(order, index, object, pred, s, c0, c1, p0, np, ob, pr);
            start = s == c0;
            if (ok && !start) {
                ok = pn_cell(order, index, object, pred, s - 1, c0, c1, p0, np, ob1, pr1);
                start = ob != ob1 || pr != pr1;
            }
            if (!ok) sbad = 1;                               // (every writer stores the same value)
        }
        const unsigned long long b = __ballot(start);
        if (lane == 0) swave[wv] = __popcll(b);
        __syncthreads();
        int pos = ng + __popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; ++w) pos += swave[w];
        if (start && pos < SKG_PAIR_NMS_MAX_GROUPS) sstart[pos] = s;
        ng += (swave[0] + swave[1]) + (swave[2] + swave[3]);
        __syncthreads();                                     // swave is read, sstart and sbad are written
    }
    const bool bad = sbad != 0;
    if (!bad && ng <= SKG_PAIR_NMS_MAX_GROUPS) {             // uniform
        if (tid == 0) sstart[ng] = c1;
        __syncthreads();
        int longest = 0;
        for (int g = tid; g < ng; g += 256) longest = max(longest, sstart[g + 1] - sstart[g]);
        if (longest > SKG_PAIR_NMS_MAX_GROUP_CELLS) atomicMax(&slong, longest);
        __syncthreads();
    }
    const int too_long = slong;                              // 0 unless the branch above ran and found one
    if (bad || ng > SKG_PAIR_NMS_MAX_GROUPS || too_long) {   // uniform: reported, every byte of the image written once
        if (tid == 0) {
            if (bad) atomicMax(status + 2, 1);
            else if (ng > SKG_PAIR_NMS_MAX_GROUPS) atomicMax(status, ng);
            else atomicMax(status + 1, too_long);
        }
        for (int c = c0 + tid; c < c1; c += 256) keep[c] = (uint8_t)1;
        return;
    }

    // ---- phase 2: greedy suppression, one wave per group
    for (int g = wv; g < ng; g += 4) {                       // uniform over the wave
        const int gs = sstart[g], n = sstart[g + 1] - gs;
        unsigned alive = 0u;                                 // bit k: this lane's cell k * 64 + lane is neither dropped nor suppressed
        int64_t pj[PN_SLOTS];
#pragma unroll
        for (int k = 0; k < PN_SLOTS; ++k) {
            const int j = k * 64 + lane;
            pj[k] = 0;
            if (j < n) {
                const int64_t c = order[gs + j];
                pj[k] = (int64_t)p0 + index[c];
                const float s = scores[c];
                if (s == s) alive |= 1u << k;                // a NaN score: dropped, suppresses nothing
            }
        }
        for (int i = 0; i + 1 < n; ++i) {                    // uniform over the wave
            const unsigned owner = __shfl(alive, i & 63, 64);
            if (!((owner >> (i >> 6)) & 1u)) continue;       // uniform: dropped or suppressed, suppresses nothing
            const int64_t pi = (int64_t)p0 + index[order[gs + i]];
            const float4 hi = *reinterpret_cast<const float4*>(boxes_h + 4 * pi);
            const float4 oi = *reinterpret_cast<const float4*>(boxes_o + 4 * pi);
#pragma unroll
            for (int k = 0; k < PN_SLOTS; ++k) {
                const int j = k * 64 + lane;
                if (j <= i || j >= n || !((alive >> k) & 1u)) continue;
                const float ih = skg_iou(hi, *reinterpret_cast<const float4*>(boxes_h + 4 * pj[k]));
                const float io = skg_iou(oi, *reinterpret_cast<const float4*>(boxes_o + 4 * pj[k]));
                // min: fminf(ih, io) > thresh where both are numbers; a NaN on either side makes it false
                const bool over = measure == SKG_PAIR_NMS_PRODUCT ? ih * io > thresh : (ih > thresh && io > thresh);
                if (over) alive &= ~(1u << k);
            }
        }
#pragma unroll
        for (int k = 0; k < PN_SLOTS; ++k) {
            const int j = k * 64 + lane;
            if (j < n) keep[order[gs + j]] = (uint8_t)((alive >> k) & 1u);
        }
    }
}

extern "C" int skg_hoi_pair_nms_u8(const float* boxes_h, const float* boxes_o, const int64_t* object, const int32_t* pair_off,
                                   const int64_t* index, const int64_t* pred, const float* scores, const int32_t* cell_off,
                                   int n_images, const int64_t* order, int measure, float thresh, uint8_t* keep,
                                   int32_t* status, void* stream) {
    if (n_images < 0 || (measure != SKG_PAIR_NMS_MIN && measure != SKG_PAIR_NMS_PRODUCT)) return SKG_E_ARG;
    if (n_images == 0) return 0;
    if (!boxes_h || !boxes_o || !object || !pair_off || !index || !pred || !scores || !cell_off || !order || !keep || !status)
        return SKG_E_ARG;
    if (!skg_aligned16(boxes_h) || !skg_aligned16(boxes_o)) return SKG_E_ALIGN;
    hipLaunchKernelGGL(skg_hoi_pair_nms_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, boxes_h, boxes_o, object,
                       pair_off, index, pred, scores, cell_off, order, measure, thresh, keep, status);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ top-k per image
// Score threshold and top-k over the scored cells of an image -- the last stage of a detector's post-processing (threshold,
// NMS, detections per image).  Not part of the reference, which ranks every cell: opt-in, this project's own rule, stated in
// include/skghoi.h (skg_hoi_topk_u8) -- parity unpinned.  One workgroup of 256 lanes per image, any number of cells.  A cell is
// a candidate iff keep_in admits it, its score is a number and score >= thresh; its key is ev_orderable(score + 0.f), so the
// keys order like the floats and -0 equals +0.  Sweep 1 counts the candidates; an image with at most k of them keeps them all.
// Otherwise a radix select, most significant byte first: four sweeps over the image (in L2 after the first), each one an LDS
// histogram of the byte over the candidates that share the prefix found so far, then the first wave scans the 256 bins from
// the top and picks the bin of the k-th largest key.  That gives T, the key of the k-th candidate, and `above`, the candidates
// over it.  The last sweep goes in arrival order in chunks of 256: key > T is kept, and of the cells with key == T the first
// k - above -- an exclusive count of the equal flags over the chunk (ballot and popcount in a wave, the four wave totals through
// LDS) on top of a base carried from chunk to chunk.  Every loop bound and every branch around a barrier is uniform and there
// is no return in front of one; counters are 32 bits (cell_off is); the histogram takes integer LDS atomics only, whose sums
// do not depend on their order, so the bytes are the same on every run.  LDS: 1 KB + a few words.
__device__ __forceinline__ bool tk_candidate(const float* __restrict__ scores, const uint8_t* __restrict__ keep_in, uint32_t i,
                                             float thresh, uint32_t& key) {
    const float s = scores[i];
    key = ev_orderable(s + 0.f);
    return (keep_in == nullptr || keep_in[i] != 0) && s == s && s >= thresh;
}

__global__ __launch_bounds__(256) void skg_hoi_topk_kernel(const float* __restrict__ scores, const int32_t* __restrict__ cell_off,
                                                           int k, float thresh, const uint8_t* __restrict__ keep_in,
                                                           uint8_t* __restrict__ keep, int32_t* __restrict__ kept) {
    __shared__ uint32_t hist[256];                           // bin b: the candidates whose byte is 255 - b (the largest first)
    __shared__ uint32_t swave[4];
    __shared__ uint32_t sel[2];                              // the chosen bin, the candidates in the bins in front of it
    const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c0 = cell_off[a], c1 = cell_off[a + 1];
    const uint32_t n = c1 > c0 ? (uint32_t)(c1 - c0) : 0u;   // the same in every lane, like everything derived from it
    scores += c0; keep += c0;
    if (keep_in) keep_in += c0;

    // ---- sweep 1: the candidates of the image
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n; i += 256) {
        uint32_t key;
        mine += tk_candidate(scores, keep_in, i, thresh, key) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if (lane == 0) swave[wv] = mine;
    __syncthreads();
    const uint32_t total = (swave[0] + swave[1]) + (swave[2] + swave[3]);
    __syncthreads();                                         // swave is read: the last sweep writes it again

    if (total <= (uint32_t)k) {                              // uniform: nothing to cut (an image without cells too)
        for (uint32_t i = tid; i < n; i += 256) {
            uint32_t key;
            keep[i] = tk_candidate(scores, keep_in, i, thresh, key) ? (uint8_t)1 : (uint8_t)0;
        }
        if (tid == 0) kept[a] = (int32_t)total;
    } else {
        // ---- radix select: the key of the k-th largest candidate
        uint32_t prefix = 0, known = 0;                      // its bytes found so far, their mask
        uint32_t need = (uint32_t)k;                         // its rank among the candidates that share the prefix, from 1
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < n; i += 256) {
                uint32_t key;
                if (tk_candidate(scores, keep_in, i, thresh, key) && (key & known) == prefix)
                    atomicAdd(&hist[255u - ((key >> shift) & 255u)], 1u);
            }
            __syncthreads();
            if (wv == 0) {                                   // the first wave: four bins per lane, a scan over the lanes
                const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
                const uint32_t sum = (h0 + h1) + (h2 + h3);
                uint32_t incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t up = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += up;
                }
                uint32_t front = incl - sum;
                if (front < need && need <= incl) {          // exactly one lane: the bin of the need-th largest is one of its four
                    uint32_t b = 4 * lane;
                    if (need > front + h0) { front += h0; ++b;
                        if (need > front + h1) { front += h1; ++b;
                            if (need > front + h2) { front += h2; ++b; } } }
                    sel[0] = b; sel[1] = front;
                }
            }
            __syncthreads();
            need -= sel[1];
            prefix |= (255u - sel[0]) << shift;
            known |= 255u << shift;
        }
        // prefix is T; k - need candidates lie above it, and the first `need` of the equal ones are wanted (need >= 1)

        // ---- last sweep, in arrival order: key > T, and the first `need` cells with key == T
        uint32_t base = 0;                                   // the equal cells in the chunks so far
        for (uint32_t i0 = 0; i0 < n; i0 += 256) {           // uniform
            const uint32_t i = i0 + tid;
            uint32_t key = 0;
            const bool cand = i < n && tk_candidate(scores, keep_in, i, thresh, key);
            const bool equal = cand && key == prefix;
            const unsigned long long b = __ballot(equal);
            if (lane == 0) swave[wv] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t pos = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; ++w) pos += swave[w];
            if (i < n) keep[i] = (cand && (key > prefix || (equal && pos < need))) ? (uint8_t)1 : (uint8_t)0;
            base += (swave[0] + swave[1]) + (swave[2] + swave[3]);
            __syncthreads();                                 // swave is read
        }
        if (tid == 0) kept[a] = k;
    }
}

extern "C" int skg_hoi_topk_u8(const float* scores, const int32_t* cell_off, int n_images, int k, float score_thresh,
                               const uint8_t* keep_in, uint8_t* keep, int32_t* kept, void* stream) {
    if (n_images < 0 || k <= 0 || score_thresh != score_thresh) return SKG_E_ARG;
    if (n_images == 0) return 0;
    if (!scores || !cell_off || !keep || !kept) return SKG_E_ARG;
    if ((((uintptr_t)scores) | ((uintptr_t)cell_off) | ((uintptr_t)kept)) & 3u) return SKG_E_ALIGN;
    hipLaunchKernelGGL(skg_hoi_topk_kernel, dim3(n_images), dim3(256), 0, (hipStream_t)stream, scores, cell_off, k, score_thresh,
                       keep_in, keep, kept);
    return skg_launch_status();
}

// ------------------------------------------------------------------------------------------------ bootstrap AP
// AP of every class in every replicate of a paired image-level bootstrap.  Not part of the reference: this project's own
// definition, the rule is stated in include/skghoi.h (skg_eval_ap_boot_f64) -- parity unpinned, there is nothing to be on a par
// with.  The ranking (labels_sorted / class_off of the two AP kernels above, img_sorted beside it) is shared by all replicates;
// a replicate counts cell i w = weights[img_sorted[i], b] times.  One wave per (class, 64 replicates), lane = replicate: the
// position in the class is the same in every lane, so the label and the image id are wave-uniform loads and the weight load
// is 64 consecutive bytes of one row.  Every lane walks the class in sequence with its running sums (int64) in registers;
// EVB_CHUNK cells are fetched ahead of the arithmetic.  A division is needed only where w * label > 0: behind a true positive
// the precision only falls until the next one, so every maximum of the precision sits on a true positive.  '11P' is one
// forward walk with eleven running maxima; 'AUC' is a forward walk for the class totals and a backward walk that carries the
// suffix maximum.  No LDS, no barrier, no atomics but atomicMax into status; every lane with a replicate stores its ap once.
#define EVB_CHUNK 8

// cell `i` of the class in replicate `b`: its weight (0 for an image id outside [0, n_images), reported through `bad`) and
// whether it is a true positive.  i, and so the image id and the branch on it, are wave-uniform.
__device__ __forceinline__ int evb_cell(const float* __restrict__ labels_sorted, const int32_t* __restrict__ img_sorted,
                                        const uint8_t* __restrict__ weights, int64_t i, int n_images, int64_t ldw, int b,
                                        bool& pos, bool& bad) {
    const int32_t img = img_sorted[i];
    pos = labels_sorted[i] != 0.f;
    if ((uint32_t)img >= (uint32_t)n_images) { bad = true; return 0; }       // checked before anything is read through it
    return (int)weights[(int64_t)img * ldw + b];
}

template <int kAlgorithm>
__global__ __launch_bounds__(64) void skg_eval_ap_boot_kernel(
    const float* __restrict__ labels_sorted, const int32_t* __restrict__ img_sorted, const int64_t* __restrict__ class_off,
    int64_t n_cells, int n_classes, const uint8_t* __restrict__ weights, int n_images, int n_boot, int64_t ldw,
    const int64_t* __restrict__ num_gt_boot, const double* __restrict__ thr, double* __restrict__ ap,
    int32_t* __restrict__ status) {
    const int c = blockIdx.x;
    const int b = blockIdx.y * 64 + (int)threadIdx.x;
    const bool live = b < n_boot;
    const int br = live ? b : n_boot - 1;                    // lanes past the last replicate read the last one, store nothing
    int64_t s0 = class_off[c], s1 = class_off[c + 1];
    if (s0 < 0) s0 = 0;
    if (s1 > n_cells) s1 = n_cells;                          // a malformed table reads nothing outside the cells
    const int64_t ngi = num_gt_boot[(int64_t)c * n_boot + br];
    const double ng = (double)ngi;
    bool bad = false;
    double result = 0.0;
    if (kAlgorithm == 0) {
        double t[11], best[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) { t[k] = thr[k]; best[k] = 0.0; }
        int64_t tp = 0, n = 0;
        for (int64_t i0 = s0; i0 < s1; i0 += EVB_CHUNK) {    // uniform
            int w[EVB_CHUNK];
            bool pos[EVB_CHUNK];
#pragma unroll
            for (int u = 0; u < EVB_CHUNK; ++u) {
                w[u] = 0; pos[u] = false;
                if (i0 + u < s1) w[u] = evb_cell(labels_sorted, img_sorted, weights, i0 + u, n_images, ldw, br, pos[u], bad);
            }
#pragma unroll
            for (int u = 0; u < EVB_CHUNK; ++u) {
                n += w[u];
                if (pos[u] && w[u] > 0 && ngi > 0) {         // pos is uniform, w is the lane's
                    tp += w[u];
                    const double prec = (double)tp / (double)n, rec = (double)tp / ng;
#pragma unroll
                    for (int k = 0; k < 11; ++k)
                        if (rec >= t[k] && prec > best[k]) best[k] = prec;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 11; ++k) result += best[k] / 11.0;       // the host meter's sequence
    } else {
        int64_t tp = 0, n = 0;                               // the class's totals in this replicate
        for (int64_t i0 = s0; i0 < s1; i0 += EVB_CHUNK) {
            int w[EVB_CHUNK];
            bool pos[EVB_CHUNK];
#pragma unroll
            for (int u = 0; u < EVB_CHUNK; ++u) {
                w[u] = 0; pos[u] = false;
                if (i0 + u < s1) w[u] = evb_cell(labels_sorted, img_sorted, weights, i0 + u, n_images, ldw, br, pos[u], bad);
            }
#pragma unroll
            for (int u = 0; u < EVB_CHUNK; ++u) { n += w[u]; if (pos[u]) tp += w[u]; }
        }
        double mx = 0.0, acc = 0.0;                          // suffix maximum of the precision; sum of w * label * maximum
        for (int64_t e = s1; e > s0; e -= EVB_CHUNK) {       // from the end: position e - 1 - u
            int w[EVB_CHUNK];
            bool pos[EVB_CHUNK];
#pragma unroll
            for (int u = 0; u < EVB_CHUNK; ++u) {
                w[u] = 0; pos[u] = false;
                if (e - 1 - u >= s0) w[u] = evb_cell(labels_sorted, img_sorted, weights, e - 1 - u, n_images, ldw, br, pos[u], bad);
            }
#pragma unroll
            for (int u = 0; u < EVB_CHUNK; ++u) {
                if (pos[u] && w[u] > 0) {
                    mx = fmax(mx, (double)tp / (double)n);
                    const double term = (double)w[u] * mx;   // rounded on its own (-ffp-contract=off), then added
                    acc += term;
                    tp -= w[u];
                }
                n -= w[u];
            }
        }
        result = ngi > 0 ? acc / ng : 0.0;
    }
    if (bad && threadIdx.x == 0) atomicMax(status, 1);
    if (live) ap[(int64_t)b * n_classes + c] = result;       // also 0 for a class without cells or without ground truth
}

extern "C" int skg_eval_ap_boot_f64(const float* labels_sorted, const int32_t* img_sorted, const int64_t* class_off,
                                    int64_t n_cells, int n_classes, const uint8_t* weights, int n_images, int n_boot,
                                    int64_t ldw, const int64_t* num_gt_boot, int algorithm, const double* thresholds11,
                                    double* ap, int32_t* status, void* stream) {
    if (n_classes < 0 || n_cells < 0 || n_boot < 1 || n_images < 0 || ldw < n_boot) return SKG_E_ARG;
    if (algorithm != SKG_AP_11P && algorithm != SKG_AP_AUC) return SKG_E_ARG;
    if (algorithm == SKG_AP_11P && !thresholds11) return SKG_E_ARG;
    if (!class_off || !num_gt_boot || !ap || !status) return SKG_E_ARG;
    if (n_cells > 0 && (!labels_sorted || !img_sorted || !weights)) return SKG_E_ARG;
    if ((n_boot + 63) / 64 > 65535) return SKG_E_LIMIT;
    if (n_classes == 0 || n_cells == 0) return 0;            // nothing to rank: nothing launched, ap stays the caller's
    const dim3 grid(n_classes, (n_boot + 63) / 64);
    if (algorithm == SKG_AP_11P)
        hipLaunchKernelGGL(skg_eval_ap_boot_kernel<0>, grid, dim3(64), 0, (hipStream_t)stream, labels_sorted, img_sorted,
                           class_off, n_cells, n_classes, weights, n_images, n_boot, ldw, num_gt_boot, thresholds11, ap, status);
    else
        hipLaunchKernelGGL(skg_eval_ap_boot_kernel<1>, grid, dim3(64), 0, (hipStream_t)stream, labels_sorted, img_sorted,
                           class_off, n_cells, n_classes, weights, n_images, n_boot, ldw, num_gt_boot, thresholds11, ap, status);
    return skg_launch_status();
}
