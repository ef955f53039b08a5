// Data-dependent selection on device, with no host synchronisation:
//   * CenterNet proposal decode: sigmoid / threshold / per-level top-k / box decode / class-agnostic NMS 0.9 /
//     post-NMS top-256 keeping ties  (Detic/third_party/CenterNet2/centernet/modeling/dense_heads/centernet.py:603-745,
//     compute_grids :321-339, layers/ml_nms.py:4-31)
//   * detectron2 fast_rcnn_inference (threshold, per-class NMS, top-k) used for the final detections
//     (Detic/detic/modeling/roi_heads/detic_roi_heads.py:214-221) and for the memory update
//     (Detic/detic/modeling/meta_arch/custom_rcnn.py:862-869)
//
// Every list has a fixed capacity and a device-side count.  Ordering is made total and deterministic with
// 64-bit keys  (float bits of the score) << 32 | ~index : descending key order == descending score, ties ->
// lower original index first (the rule the CPU oracle uses where upstream is implementation-defined).
// Sorting is an in-LDS bitonic network (<= 16384 keys = 128 KiB of the 160 KiB LDS).  NMS runs in the SAME workgroup right behind
// the sort (one launch per selection): the sorted list is walked in chunks of 64; a chunk's boxes are tested against the boxes kept
// so far (16 waves share the kept list) and against each other (64x64-bit diagonal block, resolved in the registers of one wave),
// and the walk stops as soon as the requested number of boxes has been kept -- exactly the greedy NMS of the suppression-matrix
// form, without the [n, n/64] matrix, its launch and the scan's launch.
#include "eod_common.h"
#include "../../include/eod_hip.h"
#include <algorithm>

// In-kernel phase stamps (diagnostics; compiled in only with -DEOD_STAMPS, see tools/select_stamps.py): thread 0 of workgroup 0 writes
// the 100 MHz wall clock at named points of the two single-workgroup selection kernels.
#ifdef EOD_STAMPS
__device__ unsigned long long eod_stamps[64];
#define EOD_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) eod_stamps[i] = wall_clock64(); } while (0)
extern "C" int eod_debug_read_stamps(unsigned long long* out64) {
  return hipMemcpyFromSymbol(out64, HIP_SYMBOL(eod_stamps), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : -3;
}
#else
#define EOD_STAMP(i)
#endif

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 make_key(float score, unsigned idx) {
  return ((u64)__float_as_uint(score) << 32) | (u64)(0xFFFFFFFFu - idx);
}
__device__ __forceinline__ unsigned key_index(u64 k) { return 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull); }
__device__ __forceinline__ float key_score(u64 k) { return __uint_as_float((unsigned)(k >> 32)); }

// Descending bitonic sort of 1024*E keys held E per thread: thread t owns elements [t*E, t*E + E) of the
// sequence.  Of the log2(N)(log2(N)+1)/2 compare-exchange stages only those with partner distance j >= 64*E need
// the LDS exchange buffer and barriers (10 of 91 stages for N = 8192); distances E <= j < 64*E are wave shuffles
// and j < E stay inside the thread's registers.  Block size must be 1024.
template <int E, int J>
__device__ __forceinline__ void sort_stage_intra(u64 (&v)[E], int base_i, int k) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if ((e & J) == 0) {
      const bool desc = ((base_i + e) & k) == 0;
      const u64 a = v[e], b = v[e | J];
      const bool sw = desc ? (a < b) : (a > b);
      v[e] = sw ? b : a;
      v[e | J] = sw ? a : b;
    }
  }
}

template <int E>
__device__ void block_sort_desc_reg(u64 (&v)[E], u64* xch) {
  const int t = threadIdx.x;
  const int base_i = t * E;
  constexpr int N = 1024 * E;
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j < E) {
        if (j == 1) sort_stage_intra<E, 1>(v, base_i, k);
        else if (j == 2) sort_stage_intra<E, 2>(v, base_i, k);
        else if (j == 4) sort_stage_intra<E, (E > 4 ? 4 : 1)>(v, base_i, k);
        else sort_stage_intra<E, (E > 8 ? 8 : 1)>(v, base_i, k);
      } else {
        const int tj = j / E;  // partner thread = t ^ tj, same element slot
        const bool lower = (t & tj) == 0;
        if (tj >= 64) {
#pragma unroll
          for (int e = 0; e < E; ++e) xch[e * 1024 + t] = v[e];
          __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
          u64 b;
          if (tj < 64) {
            const unsigned lo = __shfl_xor((unsigned)(v[e] & 0xFFFFFFFFull), tj, 64);
            const unsigned hi = __shfl_xor((unsigned)(v[e] >> 32), tj, 64);
            b = ((u64)hi << 32) | lo;
          } else {
            b = xch[e * 1024 + (t ^ tj)];
          }
          const bool desc = ((base_i + e) & k) == 0;
          const u64 a = v[e];
          v[e] = ((a > b) == (lower == desc)) ? a : b;   // keep the max iff (lower == desc); equal keys: either
        }
        if (tj >= 64) __syncthreads();
      }
    }
  }
}

// sort the n keys of `buf` (n <= 1024 E) descending and leave them there in sorted order
template <int E>
__device__ __forceinline__ void sort_in_place(u64* buf, int n) {
  u64 v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = threadIdx.x * E + e;
    v[e] = i < n ? buf[i] : 0ull;
  }
  __syncthreads();                     // every thread holds its keys: the buffer becomes the sort's exchange buffer
  block_sort_desc_reg<E>(v, buf);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int q = threadIdx.x * E + e;
    if (q < n) buf[q] = v[e];
  }
  __syncthreads();
}

// ... with the smallest network that holds them (n <= 1024 EMAX, EMAX = 4 or 8)
template <int EMAX>
__device__ __forceinline__ void block_sort_keys(u64* buf, int n) {
  static_assert(EMAX == 4 || EMAX == 8, "the callers' buffers hold 4096 or 8192 keys");
  if (n <= 1024) sort_in_place<1>(buf, n);
  else if (n <= 2048) sort_in_place<2>(buf, n);
  else if (EMAX == 4 || n <= 4096) sort_in_place<4>(buf, n);
  else sort_in_place<EMAX>(buf, n);
}

// ------------------------------------------------------------------------------------------------------
// Steps the selection kernels share.  None of them declares LDS: the kernel owns every array and passes pointers.  The ones that
// contain a barrier (block_*, and det_write_outputs further down) are called by ALL threads of the workgroup, from workgroup-uniform
// control flow only; a wave_* step by all lanes of a wave.
// ------------------------------------------------------------------------------------------------------
// The 4096 bins of the score histograms are 2^14-wide ranges of the float bit pattern from 2^-7 up: a monotone function of the score.
__device__ __forceinline__ int score_bin(unsigned bits) {
  int bin = (int)(bits >> 14) - (int)(0x3C000000u >> 14);
  return bin < 0 ? 0 : (bin > 4095 ? 4095 : bin);
}

// Workgroup suffix sum over 4096 bins, BPT consecutive bins per thread: h[] are the counts of bins BPT t .. BPT t + BPT - 1 in the
// first 4096 / BPT threads and zero in the others.  Returns the number of candidates in the bins ABOVE this thread's; wsum[w]
// (4096 / BPT / 64 entries) is left holding the total of wave w's bins.
template <int BPT>
__device__ __forceinline__ int block_bins_above(const int (&h)[BPT], int* wsum) {
  constexpr int WAVES = 4096 / BPT / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < BPT; ++j) mine += h[j];
  int inc = mine;                                    // inclusive suffix inside the wave (towards higher lanes)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_down(inc, off, 64);
    if (lane + off < 64) inc += t;
  }
  if (lane == 0 && wave < WAVES) wsum[wave] = inc;
  __syncthreads();
  int after = 0;                                     // candidates in the bins of higher threads' waves
  for (int w = wave + 1; w < WAVES; ++w) after += wsum[w];
  return after + inc - mine;
}

// The lowest bin of hist[4096] whose suffix reaches `want` (0 when want is 0), through *sh_cut, which the kernel has zeroed before
// its last barrier.  1024 threads, thread t owns bins 4 t .. 4 t + 3.
__device__ __forceinline__ int block_hist_cut(const int* hist, int want, int* wsum, int* sh_cut) {
  const int tid = threadIdx.x;
  const int h[4] = {hist[4 * tid], hist[4 * tid + 1], hist[4 * tid + 2], hist[4 * tid + 3]};
  const int above = block_bins_above<4>(h, wsum);
  // exactly one thread finds it
  const int s3 = above + h[3], s2 = s3 + h[2], s1 = s2 + h[1], s0 = s1 + h[0];
  if (want > 0) {
    if (above < want && s3 >= want) *sh_cut = 4 * tid + 3;
    else if (s3 < want && s2 >= want) *sh_cut = 4 * tid + 2;
    else if (s2 < want && s1 >= want) *sh_cut = 4 * tid + 1;
    else if (s1 < want && s0 >= want) *sh_cut = 4 * tid;
  }
  __syncthreads();
  return *sh_cut;
}

// Greedy NMS inside a chunk of 64 boxes, by one wave: lane i holds word i of the chunk's diagonal block (bit c: box c > i is suppressed
// by box i), `removed` the boxes earlier chunks suppressed.  Returns the kept boxes of the first `lim`.
__device__ __forceinline__ u64 wave_resolve_diag(u64 diag, u64 removed, int lim) {
  u64 kept = 0;
  for (int i = 0; i < lim; ++i) {
    // i is wave-uniform: v_readlane into scalar registers instead of an LDS-crossbar shuffle per step
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(diag & 0xFFFFFFFFull), i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(diag >> 32), i);
    if (!((removed >> i) & 1ull)) {
      kept |= 1ull << i;
      removed |= ((u64)hi << 32) | lo;
    }
  }
  return kept;
}

// Ballot compaction, one key per thread and call: the keys with `in` are appended to the LDS list `buf` through its counter *sh_n
// (one atomic per wave; the order of the list is not defined, it is sorted next).  Every lane of the wave calls it; no barrier inside.
__device__ __forceinline__ void wave_compact_key(bool in, u64 key, int* sh_n, u64* buf) {
  const int lane = threadIdx.x & 63;
  const u64 bal = __ballot(in);
  int base = 0;
  if (lane == 0 && bal) base = atomicAdd(sh_n, __popcll(bal));
  base = __shfl(base, 0, 64);
  if (in) buf[base + __popcll(bal & ((1ull << lane) - 1ull))] = key;
}

// ------------------------------------------------------------------------------------------------------
// NMS on a score-sorted list, by the workgroup that sorted it
// ------------------------------------------------------------------------------------------------------
struct ScanOut {
  // gathered outputs (any may be null)
  float* out_boxes;
  float* out_scores;
  int* out_labels;
  int* out_rows;
  int* out_count;
  int cap;
  // optional: torch.unique of out_rows (ascending, custom_rcnn.py:875) and its length
  int* uniq_rows;
  int* uniq_count;
  int uniq_cap;
  // optional: groups of kept entries that share one source row (= one class-agnostic box): rep_of[r] = first kept entry with
  // the row of entry r; rep_list = the entries that are their own representative, ascending; rep_count = their number
  int* rep_of;
  int* rep_list;
  int* rep_count;
};

// scene b of a batch: every output is `batch` single-scene buffers back to back
__device__ __forceinline__ ScanOut scene_outputs(ScanOut o, int b) {
  if (o.out_boxes) o.out_boxes += (size_t)b * o.cap * 4;
  if (o.out_scores) o.out_scores += (size_t)b * o.cap;
  if (o.out_labels) o.out_labels += (size_t)b * o.cap;
  if (o.out_rows) o.out_rows += (size_t)b * o.cap;
  if (o.out_count) o.out_count += b;
  if (o.uniq_rows) o.uniq_rows += (size_t)b * o.uniq_cap;
  if (o.uniq_count) o.uniq_count += b;
  if (o.rep_of) o.rep_of += (size_t)b * o.cap;
  if (o.rep_list) o.rep_list += (size_t)b * o.cap;
  if (o.rep_count) o.rep_count += b;
  return o;
}

#define NMS_KEPT_MAX 512

struct NmsSmem {
  float kb[NMS_KEPT_MAX * 4];   // kept boxes, in keep order
  int kidx[NMS_KEPT_MAX];       // their position in the sorted list
  float cb[64 * 4];             // the chunk's boxes
  float cs[64];                 // the chunk's scores (the tie rule of the last chunks reads them one by one)
  u64 diag[64];                 // bit c of word i: chunk box c (c > i) is suppressed by chunk box i
  u64 supp;                     // bit i: chunk box i is suppressed by a box kept in an earlier chunk
  int total, stop;
  float kth;
};

__device__ __forceinline__ bool iou_over(float x1, float y1, float x2, float y2, float area_i, float a1, float b1, float a2, float b2,
                                         float thr) {
  const float w = fmaxf(fminf(x2, a2) - fmaxf(x1, a1), 0.f);
  const float h = fmaxf(fminf(y2, b2) - fmaxf(y1, b1), 0.f);
  const float inter = w * h;
  const float area_j = (a2 - a1) * (b2 - b1);
  const float iou = inter / (area_i + area_j - inter);
  return iou > thr;
}

// Class-agnostic greedy NMS over the first n entries of a score-sorted list (boxes / scores in global memory, written by this
// workgroup before the call) + gather of the kept entries (boxes, scores, count).  Every kept box whose score equals the score of
// kept box #max_keep is kept too (centernet.py:733-741, ">= kth").  Returns whether the walk ended by that rule (and not because the
// list ran out).  Block = 1024 threads.
__device__ bool block_greedy_nms(const float* __restrict__ boxes, const float* __restrict__ scores, int n, float thr, int max_keep,
                                 const ScanOut& o, NmsSmem* S) {
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
  if (tid == 0) {
    S->total = 0;
    S->stop = 0;
    S->kth = -1.0f;
  }
  __syncthreads();
  const int nchunk = (n + 63) >> 6;
  // wave 0 holds the NEXT chunk's boxes / scores in registers: its global loads are issued a whole chunk ahead instead of
  // at the top of the chunk that needs them (one L2 round trip per chunk off the serial path)
  float nb0 = 0.f, nb1 = 0.f, nb2 = 0.f, nb3 = 0.f, nsc = 0.f;
  auto fetch = [&](int c) {
    const int j = c * 64 + tid;
    if (tid < 64 && j < n) {
      nb0 = boxes[j * 4 + 0]; nb1 = boxes[j * 4 + 1]; nb2 = boxes[j * 4 + 2]; nb3 = boxes[j * 4 + 3];
      nsc = scores[j];
    }
  };
  fetch(0);
  for (int c = 0; c < nchunk; ++c) {
    const int lim = min(64, n - c * 64);
    if (tid < 64) {
      if (tid < lim) {
        S->cb[tid * 4 + 0] = nb0;
        S->cb[tid * 4 + 1] = nb1;
        S->cb[tid * 4 + 2] = nb2;
        S->cb[tid * 4 + 3] = nb3;
        S->cs[tid] = nsc;
      }
      S->diag[tid] = 0;
      if (tid == 0) S->supp = 0;
    }
    if (c + 1 < nchunk) fetch(c + 1);
    __syncthreads();
    const int total0 = S->total;
    const int nk = total0 < NMS_KEPT_MAX ? total0 : NMS_KEPT_MAX;
    const bool valid = lane < lim;
    float a1 = 0.f, b1 = 0.f, a2 = 0.f, b2 = 0.f;
    if (valid) {
      a1 = S->cb[lane * 4 + 0]; b1 = S->cb[lane * 4 + 1]; a2 = S->cb[lane * 4 + 2]; b2 = S->cb[lane * 4 + 3];
    }
    // (A) against the boxes kept in earlier chunks: wave `grp` takes kept boxes grp, grp + 16, ...
    bool sup = false;
    if (valid) {
      for (int j = grp; j < nk; j += 16) {
        const float x1 = S->kb[j * 4 + 0], y1 = S->kb[j * 4 + 1], x2 = S->kb[j * 4 + 2], y2 = S->kb[j * 4 + 3];
        const float area_i = (x2 - x1) * (y2 - y1);
        if (iou_over(x1, y1, x2, y2, area_i, a1, b1, a2, b2, thr)) {
          sup = true;
          break;
        }
      }
    }
    const u64 bal = __ballot(sup);
    if (lane == 0 && bal) atomicOr(&S->supp, bal);
    // (B) inside the chunk: lane = suppressor i, wave `grp` takes the later boxes grp*4 .. grp*4+3
    if (valid) {
      u64 bits = 0;
      const float area_i = (a2 - a1) * (b2 - b1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c2 = grp * 4 + q;
        if (c2 > lane && c2 < lim) {
          if (iou_over(a1, b1, a2, b2, area_i, S->cb[c2 * 4 + 0], S->cb[c2 * 4 + 1], S->cb[c2 * 4 + 2], S->cb[c2 * 4 + 3], thr))
            bits |= 1ull << c2;
        }
      }
      if (bits) atomicOr(&S->diag[lane], bits);
    }
    __syncthreads();
    if (tid < 64) {
      const u64 kept = wave_resolve_diag(S->diag[tid], S->supp, lim);
      const int nkept = __popcll(kept);
      if (total0 + nkept < max_keep) {
        // fast path (every chunk but the last one): all lanes append their kept box in parallel
        if ((kept >> tid) & 1ull) {
          const int pos = total0 + __popcll(kept & ((1ull << tid) - 1ull));
          if (pos < NMS_KEPT_MAX) {
            S->kb[pos * 4 + 0] = a1; S->kb[pos * 4 + 1] = b1; S->kb[pos * 4 + 2] = a2; S->kb[pos * 4 + 3] = b2;
            S->kidx[pos] = c * 64 + tid;
          }
        }
        if (tid == 0) S->total = total0 + nkept;
      } else if (tid == 0) {
        // append kept boxes one by one, honouring max_keep and the ties
        int total = total0;
        int stop = 0;
        float kth = S->kth;
        for (int i = 0; i < lim; ++i) {
          if (!((kept >> i) & 1ull)) continue;
          const int idx = c * 64 + i;
          if (total >= max_keep && !(S->cs[i] >= kth)) {
            // boxes after this one have lower-or-equal score; they may still be equal only if scores[idx] >= kth, which failed ->
            // everything later is strictly lower: stop
            stop = 1;
            break;
          }
          if (total < NMS_KEPT_MAX) {
            S->kb[total * 4 + 0] = S->cb[i * 4 + 0]; S->kb[total * 4 + 1] = S->cb[i * 4 + 1];
            S->kb[total * 4 + 2] = S->cb[i * 4 + 2]; S->kb[total * 4 + 3] = S->cb[i * 4 + 3];
            S->kidx[total] = idx;
          }
          ++total;
          if (total == max_keep) kth = S->cs[i];
        }
        S->total = total;
        S->kth = kth;
        // if the list is full and the next chunk starts below kth, stop
        if (!stop && total >= max_keep) {
          const int nxt = (c + 1) * 64;
          if (nxt >= n || scores[nxt] < kth) stop = 1;
        }
        S->stop = stop;
      }
    }
    __syncthreads();
#ifdef EOD_STAMPS
    if (threadIdx.x == 0 && blockIdx.x == 0) eod_stamps[6] = (unsigned long long)(c + 1);      // chunks walked
#endif
    if (S->stop) break;
  }
  __syncthreads();
  EOD_STAMP(5);
  const bool stopped = S->stop != 0;      // the walk ended on its own rule, not because the list ran out
  int total = S->total;
  if (total > o.cap) total = o.cap;
  if (total > NMS_KEPT_MAX) total = NMS_KEPT_MAX;
  if (tid == 0 && o.out_count) *o.out_count = total;
  for (int r = tid; r < total; r += blockDim.x) {
    const int idx = S->kidx[r];
    if (o.out_boxes) {
      o.out_boxes[r * 4 + 0] = S->kb[r * 4 + 0];
      o.out_boxes[r * 4 + 1] = S->kb[r * 4 + 1];
      o.out_boxes[r * 4 + 2] = S->kb[r * 4 + 2];
      o.out_boxes[r * 4 + 3] = S->kb[r * 4 + 3];
    }
    if (o.out_scores) o.out_scores[r] = scores[idx];
  }
  __syncthreads();
  return stopped;
}

// ------------------------------------------------------------------------------------------------------
// CenterNet proposals
// ------------------------------------------------------------------------------------------------------
struct CnArgs {
  const float* head;
  int head_stride;
  int levels;
  int level_off[6];
  int level_w[5];
  int level_stride[5];
  float level_scale[5];
  float score_thresh;
  int topk;
  u64* cand_keys;  // packed per level: level l owns slots [pk_off[l], pk_off[l+1]), min(level size, topk) each
  int* cand_cnt;   // [levels]
  int pk_off[6];
  // batch > 1: `head` is level major over the scenes (level l of scene b = rows batch * level_off[l] + b * n_l ...), candidate keys
  // carry the scene's own position level_off[l] + i; cand_keys / cand_cnt hold `batch` sets back to back
  int batch;
};

__device__ __forceinline__ size_t cn_head_row(const CnArgs& p, int scene, int level, int i) {
  const int n = p.level_off[level + 1] - p.level_off[level];
  return (size_t)p.batch * p.level_off[level] + (size_t)scene * n + i;
}

// The box of position g (scene-local, on `level`) from the head's four regression outputs (centernet.py:321-339, 660-672).  `p` is the
// kernel's own argument struct and `scene` the workgroup's scene: the head is the one operand no kernel offsets by its scene.
__device__ __forceinline__ float4 cn_decode_box(const CnArgs& p, int scene, int level, int g) {
  const int i = g - p.level_off[level];
  const int w = p.level_w[level];
  const int stride = p.level_stride[level];
  const int gy_i = i / w, gx_i = i - gy_i * w;
  const float gx = (float)(gx_i * stride + stride / 2);
  const float gy = (float)(gy_i * stride + stride / 2);
  const float* h = p.head + cn_head_row(p, scene, level, i) * p.head_stride;
  const float sc = p.level_scale[level];
  const float st = (float)stride;
  const float r0 = fmaxf(h[1] * sc, 0.f) * st;
  const float r1 = fmaxf(h[2] * sc, 0.f) * st;
  const float r2 = fmaxf(h[3] * sc, 0.f) * st;
  const float r3 = fmaxf(h[4] * sc, 0.f) * st;
  const float x1 = gx - r0, y1 = gy - r1;
  float x2 = gx + r2, y2 = gy + r3;
  x2 = fmaxf(x2, x1 + 0.01f);
  y2 = fmaxf(y2, y1 + 0.01f);
  return make_float4(x1, y1, x2, y2);
}

#define EOD_SORT_MAX 16384

// Sorts the n <= 1024 E keys of `buf` (descending) and writes the best `take` of them as (sqrt(score), global position) keys into
// the level's packed candidate slots; the remaining slots are zeroed.
template <int E>
__device__ __forceinline__ void cn_sort_emit(u64* buf, int n, int take, int r0, int slots, u64* __restrict__ out) {
  u64 v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = threadIdx.x * E + e;
    v[e] = i < n ? buf[i] : 0ull;
  }
  __syncthreads();
  block_sort_desc_reg<E>(v, buf);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int r = threadIdx.x * E + e;
    if (r < slots) {
      u64 k = 0;
      if (r < take) k = make_key(sqrtf(key_score(v[e])), (unsigned)(r0 + (int)key_index(v[e])));
      out[r] = k;
    }
  }
}

// one block per level: per-level top-k by score.  Only the candidates that can be among the best `topk` are sorted: a 4096-bin
// histogram of the score bits gives the lowest bin b* whose suffix holds >= topk candidates (scores are sigmoids in (0, 1): the
// bins are 2^14-wide ranges of the float bit pattern, a monotone function of the score), the keys of the bins >= b* are compacted
// and a sort of just their number (1024 / 2048 / 4096 / ... keys) follows -- at 640x640 the 6400 positions of the finest level
// pass the threshold almost everywhere, and a full 8192-key bitonic sort was 70 us on the frame's critical chain.
// EMAX = 8: levels up to 8192 positions, 16: up to 16384.
template <int EMAX>
__global__ __launch_bounds__(1024) void cn_level_topk_kernel(CnArgs p) {
  EOD_CHAIN_PRIO();
  __shared__ u64 xch[1024 * EMAX];
  __shared__ int hist[4096];
  __shared__ int wsum[16];
  __shared__ int sh_cnt, sh_cut, sh_n2;
  const int level = blockIdx.x, scene = blockIdx.y;
  const int r0 = p.level_off[level];
  const int n = p.level_off[level + 1] - r0;
  const size_t head0 = cn_head_row(p, scene, level, 0);
  // (the argument struct is not written to: a modified copy lives in scratch memory -- 168 bytes per lane -- and every indexed
  // read of the level tables goes through it)
  u64* const cand_keys = p.cand_keys + (size_t)scene * p.pk_off[p.levels];
  int* const cand_cnt = p.cand_cnt + scene * 8;
  const int tid = threadIdx.x;
  for (int i = tid; i < 4096; i += 1024) hist[i] = 0;
  if (tid == 0) {
    sh_cnt = 0;
    sh_cut = 0;
    sh_n2 = 0;
  }
  __syncthreads();
  u64 v[EMAX];
  int local = 0;
#pragma unroll
  for (int e = 0; e < EMAX; ++e) {
    const int i = e * 1024 + tid;
    u64 k = 0;
    if (i < n) {
      const float heat = eod_sigmoid_precise(p.head[(head0 + i) * p.head_stride]);
      if (heat > p.score_thresh) {
        k = make_key(heat, (unsigned)i);
        atomicAdd(&hist[score_bin(__float_as_uint(heat))], 1);
        ++local;
      }
    }
    v[e] = k;
  }
  if (local) atomicAdd(&sh_cnt, local);
  __syncthreads();
  const int cnt = sh_cnt;
  const int take = cnt < p.topk ? cnt : p.topk;
  const int cut = block_hist_cut(hist, take, wsum, &sh_cut);
#pragma unroll
  for (int e = 0; e < EMAX; ++e) wave_compact_key(v[e] != 0 && score_bin((unsigned)(v[e] >> 32)) >= cut, v[e], &sh_n2, xch);
  __syncthreads();
  const int n2 = sh_n2;                              // take <= n2 <= cnt
  const int slots = p.pk_off[level + 1] - p.pk_off[level];
  u64* out = cand_keys + p.pk_off[level];
  const int ns = n2 > slots ? n2 : slots;            // the sort's size must also cover the slots it zero-fills
  if (ns <= 1024) cn_sort_emit<1>(xch, n2, take, r0, slots, out);
  else if (ns <= 2048) cn_sort_emit<2>(xch, n2, take, r0, slots, out);
  else if (ns <= 4096) cn_sort_emit<4>(xch, n2, take, r0, slots, out);
  else if (EMAX <= 8 || ns <= 8192) cn_sort_emit<8>(xch, n2, take, r0, slots, out);
  else cn_sort_emit<(EMAX > 8 ? 16 : 8)>(xch, n2, take, r0, slots, out);
  if (tid == 0) cand_cnt[level] = take;
}

// single block: merge the per-level lists, sort by sqrt-score, decode boxes (E*1024 >= packed slots: E = 4 covers the usual
// 1000 + 1000 + <=1000 + ... <= 4096 candidates with half the sort of E = 8), then class-agnostic NMS + post-NMS cut with ties
template <int E>
__global__ __launch_bounds__(1024) void cn_merge_nms_kernel(CnArgs p, float* sorted_boxes, float* sorted_scores, float nms_thresh,
                                                             int post_topk, ScanOut o) {
  EOD_CHAIN_PRIO();
  __shared__ u64 xch[1024 * E];
  static_assert(sizeof(NmsSmem) <= sizeof(u64) * 1024 * E, "the NMS state reuses the sort's exchange buffer");
  const int total_slots = p.pk_off[p.levels];
  const int scene = blockIdx.x;
  const u64* const cand_keys = p.cand_keys + (size_t)scene * total_slots;
  const int* const cand_cnt = p.cand_cnt + scene * 8;
  sorted_boxes += (size_t)scene * total_slots * 4;
  sorted_scores += (size_t)scene * total_slots;
  o = scene_outputs(o, scene);
  EOD_STAMP(0);
  u64 v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = threadIdx.x * E + e;
    v[e] = i < total_slots ? cand_keys[i] : 0ull;
  }
  EOD_STAMP(1);
  int n = 0;
  for (int l = 0; l < p.levels; ++l) n += cand_cnt[l];
  // Decode the boxes of the sorted keys held in `keys` (registers of a full sort, or the sorted LDS list of the best candidates)
  auto decode = [&](int r, u64 k) {
    const int g = (int)key_index(k);
    int level = 0;
    while (level + 1 < p.levels && g >= p.level_off[level + 1]) ++level;
    const float4 bx = cn_decode_box(p, scene, level, g);
    sorted_boxes[r * 4 + 0] = bx.x;
    sorted_boxes[r * 4 + 1] = bx.y;
    sorted_boxes[r * 4 + 2] = bx.z;
    sorted_boxes[r * 4 + 3] = bx.w;
    sorted_scores[r] = key_score(k);
  };
  // Fast path: NMS 0.9 keeps nearly every candidate, so the post-NMS cut (256 + ties) is reached inside the best few hundred of
  // the up to 4096.  A histogram of the score bits (as in cn_level_topk_kernel) picks the lowest bin whose suffix holds >= 1024
  // candidates; only those are sorted (1024-2048 keys instead of 4096: 35 us of this kernel were the sort) and walked.  If the
  // walk runs out of them before it stops by its own rule, the full list is sorted and walked instead (same results either way).
  __shared__ int hist[4096];
  __shared__ int wsum[16];
  __shared__ int sh_cut, sh_n2;
  if (n > 1024) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 4096; i += 1024) hist[i] = 0;
    if (tid == 0) {
      sh_cut = 0;
      sh_n2 = 0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (v[e]) atomicAdd(&hist[score_bin((unsigned)(v[e] >> 32))], 1);
    __syncthreads();
    const int cut = block_hist_cut(hist, 1024, wsum, &sh_cut);
#pragma unroll
    for (int e = 0; e < E; ++e) wave_compact_key(v[e] != 0 && score_bin((unsigned)(v[e] >> 32)) >= cut, v[e], &sh_n2, xch);
    __syncthreads();
    const int n2 = sh_n2;                            // 1024 <= n2 <= n
    if (n2 < n && n2 <= 4096) {
      block_sort_keys<4>(xch, n2);
      EOD_STAMP(2);
      for (int r = tid; r < n2; r += 1024) decode(r, xch[r]);
      __syncthreads();
      EOD_STAMP(3);
      const bool stopped = block_greedy_nms(sorted_boxes, sorted_scores, n2, nms_thresh, post_topk, o, reinterpret_cast<NmsSmem*>(xch));
      EOD_STAMP(4);
      if (stopped) return;                           // workgroup-uniform
    }
  }
  block_sort_desc_reg<E>(v, xch);
  EOD_STAMP(2);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int r = threadIdx.x * E + e;
    if (r < n) decode(r, v[e]);
  }
  __syncthreads();          // the sorted list (global) and the end of the sort's use of xch
  EOD_STAMP(3);
  block_greedy_nms(sorted_boxes, sorted_scores, n, nms_thresh, post_topk, o, reinterpret_cast<NmsSmem*>(xch));
  EOD_STAMP(4);
}

// ------------------------------------------------------------------------------------------------------
// CenterNet proposals, wide lists (the TRAINING thresholds: PRE / POST_NMS_TOPK_TRAIN 4000 / 2000, NMS_TH_TRAIN 0.9,
// Base-C2_L_R5021k_640b64_4x_recurrent.yaml:45-49 -> centernet.py:214-219,603-745): up to 16384 merged candidates and 4096 kept
// boxes, beyond what one workgroup's LDS holds.  Three launches behind cn_level_topk_kernel:
//   cn_rank_decode_kernel   every candidate finds its rank in the merged (sqrt-score desc, position asc) order by binary searches
//                           in the per-level lists (they are sorted already) and writes its decoded box there: a merge without a sort
//   nms_matrix_kernel       the upper triangle of the [n, n/64] suppression bit matrix, one 64 x 64 block per wave, whole chip
//   nms_scan_kernel         one workgroup per scene walks the list in chunks of 64: diagonal block resolved in one wave's registers,
//                           the kept rows OR-ed into the removed set by all 16 waves (next chunk's rows prefetched unconditionally),
//                           stops by the '>= kth' rule of centernet.py:733-741 and writes the kept boxes in order
// ------------------------------------------------------------------------------------------------------
#define WIDE_MAX_SLOTS 16384
#define WIDE_MAX_WORDS (WIDE_MAX_SLOTS / 64)
#define WIDE_MAX_CAP 4096

// number of keys of a (descending by score) level list whose score is > s (strict = 1) or >= s (strict = 0)
__device__ __forceinline__ int cn_count_above(const u64* __restrict__ keys, int n, float s, int strict) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float v = key_score(keys[mid]);
    const bool above = strict ? (v > s) : (v >= s);
    if (above) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void cn_rank_decode_kernel(CnArgs p, float* sorted_boxes, float* sorted_scores, int* n_out) {
  const int total_slots = p.pk_off[p.levels];
  const int scene = blockIdx.y;
  const u64* const cand_keys = p.cand_keys + (size_t)scene * total_slots;
  const int* const cand_cnt = p.cand_cnt + scene * 8;
  sorted_boxes += (size_t)scene * total_slots * 4;
  sorted_scores += (size_t)scene * total_slots;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s == 0) {
    int n = 0;
    for (int l = 0; l < p.levels; ++l) n += cand_cnt[l];
    n_out[scene] = n;
  }
  if (s >= total_slots) return;
  int level = 0;
  while (level + 1 < p.levels && s >= p.pk_off[level + 1]) ++level;
  if (s - p.pk_off[level] >= cand_cnt[level]) return;
  const u64 k = cand_keys[s];
  const float sc = key_score(k);
  const unsigned g = key_index(k);
  // rank = number of candidates that precede k in (score desc, position asc) order.  A level list is sorted by the HEAT; sqrt is
  // monotone, so the keys of one sqrt-score form a run [a, b) -- inside it the positions are counted one by one (two heats can share
  // a sqrt in fp32, and quantised logits give long runs)
  int rank = 0;
  for (int l = 0; l < p.levels; ++l) {
    const u64* lk = cand_keys + p.pk_off[l];
    const int nl = cand_cnt[l];
    const int a = cn_count_above(lk, nl, sc, 1), b = cn_count_above(lk, nl, sc, 0);
    rank += a;
    for (int q = a; q < b; ++q) rank += key_index(lk[q]) < g ? 1 : 0;
  }
  reinterpret_cast<float4*>(sorted_boxes)[rank] = cn_decode_box(p, scene, level, (int)g);
  sorted_scores[rank] = sc;
}

// bit (j & 63) of M[i][j >> 6], j > i: IoU(box i, box j) > thr.  Block = 4 waves = 4 column words of one 64-row block.
__global__ __launch_bounds__(256) void nms_matrix_kernel(const float* __restrict__ sorted_boxes, const int* __restrict__ n_ptr,
                                                          int total_slots, int words, float thr, u64* __restrict__ M) {
  const int scene = blockIdx.z;
  const int n = n_ptr[scene];
  const int rb = blockIdx.y, cw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (cw < rb || rb * 64 >= n || cw * 64 >= n) return;              // wave-uniform
  const float4* boxes = reinterpret_cast<const float4*>(sorted_boxes) + (size_t)scene * total_slots;
  M += (size_t)scene * total_slots * words;
  const int i = rb * 64 + lane, j = cw * 64 + lane;
  const float4 bi = i < n ? boxes[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 bj = j < n ? boxes[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
  const int jn = min(64, n - cw * 64);
  u64 bits = 0;
  for (int c = 0; c < jn; ++c) {
    const float a1 = __shfl(bj.x, c, 64), b1 = __shfl(bj.y, c, 64), a2 = __shfl(bj.z, c, 64), b2 = __shfl(bj.w, c, 64);
    if (cw * 64 + c > i && iou_over(bi.x, bi.y, bi.z, bi.w, area_i, a1, b1, a2, b2, thr)) bits |= 1ull << c;
  }
  if (i < n) M[(size_t)i * words + cw] = bits;
}

__global__ __launch_bounds__(1024) void nms_scan_kernel(const float* __restrict__ sorted_boxes, const float* __restrict__ sorted_scores,
                                                         const int* __restrict__ n_ptr, int total_slots, int words,
                                                         const u64* __restrict__ M, int max_keep, ScanOut o) {
  __shared__ u64 removed[WIDE_MAX_WORDS];
  __shared__ u64 sh_kept;
  __shared__ int sh_total, sh_stop;
  __shared__ float sh_kth;
  const int scene = blockIdx.x;
  const int n = n_ptr[scene];
  const float4* boxes = reinterpret_cast<const float4*>(sorted_boxes) + (size_t)scene * total_slots;
  const float* scores = sorted_scores + (size_t)scene * total_slots;
  M += (size_t)scene * total_slots * words;
  o = scene_outputs(o, scene);
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
  const int nw = (n + 63) >> 6;
  for (int w = tid; w < WIDE_MAX_WORDS; w += 1024) removed[w] = 0;
  if (tid == 0) {
    sh_total = 0;
    sh_stop = 0;
    sh_kth = -1.0f;
  }
  __syncthreads();
  // Every wave owns four rows of a chunk (grp, grp + 16, grp + 32, grp + 48), a lane the words c + 1 + lane + 64 q behind the
  // diagonal.  The rows of chunk c + 1 are requested before chunk c is resolved: nothing on the serial path waits for HBM.
  constexpr int Q = WIDE_MAX_WORDS / 64;
  u64 nxt[4][Q];
  u64 nd = 0;
  float nsc = 0.f;
  auto fetch = [&](int c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = c * 64 + grp + 16 * r;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int w = c + 1 + lane + 64 * q;
        nxt[r][q] = (row < n && w < nw) ? M[(size_t)row * words + w] : 0ull;
      }
    }
    if (grp == 0) {
      const int row = c * 64 + lane;
      nd = row < n ? M[(size_t)row * words + c] : 0ull;
      nsc = row < n ? scores[row] : 0.f;
    }
  };
  fetch(0);
  for (int c = 0; c < nw; ++c) {
    u64 cur[4][Q];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < Q; ++q) cur[r][q] = nxt[r][q];
    const u64 diag = nd;
    const float sc = nsc;
    if (c + 1 < nw) fetch(c + 1);
    const int lim = min(64, n - c * 64);
    if (grp == 0) {
      u64 rem = removed[c];
      if (lim < 64) rem |= ~0ull << lim;
      const u64 kept = wave_resolve_diag(diag, rem, lim);
      // the cut: the first max_keep kept boxes, then every kept box whose score equals the max_keep-th's (centernet.py:733-741)
      const int total0 = sh_total;
      const bool mine = (kept >> lane) & 1ull;
      const int r = total0 + __popcll(kept & ((1ull << lane) - 1ull));
      float kth = sh_kth;
      const u64 at_k = __ballot(mine && r == max_keep - 1);
      if (at_k) kth = __shfl(sc, __ffsll((long long)at_k) - 1, 64);
      const bool take = mine && (r < max_keep || sc >= kth);
      const u64 taken = __ballot(take);
      const bool over = __ballot(mine && !take) != 0;
      if (take && r < o.cap) {
        reinterpret_cast<float4*>(o.out_boxes)[r] = boxes[c * 64 + lane];
        o.out_scores[r] = sc;
      }
      if (lane == 0) {
        const int total = total0 + __popcll(taken);
        sh_total = total;
        sh_kth = kth;
        sh_kept = taken;
        // every later score is <= this chunk's last: past the cut only equal scores can still be taken
        int stop = over ? 1 : 0;
        if (!stop && total >= max_keep) {
          const int nx = (c + 1) * 64;
          if (nx >= n || scores[nx] < kth) stop = 1;
        }
        sh_stop = stop;
      }
    }
    __syncthreads();
    if (sh_stop) break;
    const u64 kept = sh_kept;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      u64 acc = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((kept >> (grp + 16 * r)) & 1ull) acc |= cur[r][q];
      const int w = c + 1 + lane + 64 * q;
      if (acc && w < nw) atomicOr(&removed[w], acc);
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) *o.out_count = sh_total < o.cap ? sh_total : o.cap;
}

// ------------------------------------------------------------------------------------------------------
// fast_rcnn_inference in one launch: threshold + sort + per-class NMS + top-k (+ unique rows)
// ------------------------------------------------------------------------------------------------------
// All detections of one proposal row carry the row's class-agnostic box, so per-class NMS never needs an IoU between two
// candidates: it needs the IoU between two ROWS.  The kernel builds the R x R bit matrix M (bit r' of row r: IoU(box r, box r') >
// thr) once -- one 64-bit word per thread -- and greedy NMS becomes bit tests: a candidate (row r, class c) is suppressed iff bit
// r of supp[c] is set, where supp[c] is the OR of M[r'] over the kept (r', c).  Candidates are sorted in batches: the first batch
// holds the >= 1024 best scores (histogram of the score bits, as in cn_level_topk_kernel), which is nearly always enough to keep
// `topk`; only if it is not, the rest is sorted and the walk continues (same state, same order: exactly the greedy NMS over the
// fully sorted list).  The walk itself is done by ONE wave (no workgroup barrier per chunk of 64 candidates).
#define DET_MAX_R 512
#define DET_WORDS (DET_MAX_R / 64)
#define DET_MAX_C 24

// ------------------------------------------------------------------------------------------------------
// Steps of the two fast_rcnn_inference tails (det_select_kernel, detw_tail_kernel), 1024 threads
// ------------------------------------------------------------------------------------------------------
// Row r's box clipped to the image into cbx (the zero box for the rows beyond the count, `in` false); returns whether the row is in
// use and its box finite.
__device__ __forceinline__ bool det_clip_row(const float* boxes, int r, bool in, float img_w, float img_h, float* cbx) {
  float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
  if (in) {
    b0 = boxes[r * 4 + 0]; b1 = boxes[r * 4 + 1]; b2 = boxes[r * 4 + 2]; b3 = boxes[r * 4 + 3];
  }
  cbx[r * 4 + 0] = fminf(fmaxf(b0, 0.f), img_w);
  cbx[r * 4 + 1] = fminf(fmaxf(b1, 0.f), img_h);
  cbx[r * 4 + 2] = fminf(fmaxf(b2, 0.f), img_w);
  cbx[r * 4 + 3] = fminf(fmaxf(b3, 0.f), img_h);
  return in && isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3);
}

// IoU bit matrix of the R rows in use: bit b of Mx[r][w]: IoU(box r, box 64 w + b) > thr.  One word (64 partner rows) per thread
// and step; the first `words` words of a row are written (>= ceil(R / 64): zero beyond the rows in use), no other is ever read.
__device__ __forceinline__ void det_row_iou_matrix(const float* cbx, int R, int words, float nms_thresh, u64* Mx) {
  const int W = (R + 63) >> 6;
  for (int idx = threadIdx.x; idx < R * words; idx += 1024) {
    const int r = idx / words, w = idx - r * words;
    u64 bits = 0;
    if (w < W) {
      const float x1 = cbx[r * 4 + 0], y1 = cbx[r * 4 + 1], x2 = cbx[r * 4 + 2], y2 = cbx[r * 4 + 3];
      const float area = (x2 - x1) * (y2 - y1);
      for (int b = 0; b < 64; ++b) {
        const int r2 = w * 64 + b;
        if (r2 < R && r2 != r &&
            iou_over(x1, y1, x2, y2, area, cbx[r2 * 4 + 0], cbx[r2 * 4 + 1], cbx[r2 * 4 + 2], cbx[r2 * 4 + 3], nms_thresh))
          bits |= 1ull << b;
      }
    }
    Mx[r * DET_WORDS + w] = bits;
  }
}

// Rank of every kept entry of the sorted batch buf[0, n2) in list order (keptbits: bit q = entry q survives its class's NMS; n2 <=
// 64 MAX_WORDS, MAX_WORDS = 64 or 128): popcounts of the words before it + of the bits below it.  The entries of rank < topk - total0
// go to kept_key[total0 + rank].  Returns the number of kept entries of the batch.  wordpre[MAX_WORDS] and wsum are scratch.
template <int MAX_WORDS>
__device__ __forceinline__ int block_rank_and_take(const u64* keptbits, int n2, int total0, int topk, const u64* buf, u64* kept_key,
                                                   int* wordpre, int* wsum) {
  static_assert(MAX_WORDS == 64 || MAX_WORDS == 128, "one or two waves scan the words");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwords = (n2 + 63) >> 6;
  if (tid < MAX_WORDS) {
    const int pc = tid < nwords ? __popcll(keptbits[tid]) : 0;
    int inc = pc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    wordpre[tid] = inc - pc;                               // exclusive inside the wave
    if (lane == 63) wsum[wave] = inc;
  }
  __syncthreads();
  for (int q = tid; q < n2; q += 1024) {
    const u64 wbits = keptbits[q >> 6];
    if ((wbits >> (q & 63)) & 1ull) {
      const int rank = wordpre[q >> 6] + ((q >> 6) >= 64 ? wsum[0] : 0) + __popcll(wbits & ((1ull << (q & 63)) - 1ull));
      const int pos = total0 + rank;
      if (pos < topk && pos < NMS_KEPT_MAX) kept_key[pos] = buf[q];
    }
  }
  return wsum[0] + (nwords > 64 ? wsum[1] : 0);
}

// Ballot compaction over one flag per thread of the first NMS_KEPT_MAX threads (false in the others): returns the number of set flags
// below this thread's -- its slot in the compacted list -- and the number of all of them through *all.
__device__ __forceinline__ int block_compact_flags(bool pred, int* wsum, int* all) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64 bal = 0;
  if (tid < NMS_KEPT_MAX) {
    bal = __ballot(pred);
    if (lane == 0) wsum[wave] = __popcll(bal);
  }
  __syncthreads();
  int before = 0;
  *all = 0;
#pragma unroll
  for (int w = 0; w < NMS_KEPT_MAX / 64; ++w) {
    const int cw = wsum[w];
    if (w < wave) before += cw;
    *all += cw;
  }
  return before + __popcll(bal & ((1ull << lane) - 1ull));
}

// The outputs of a selection from its kept keys (kept_key[0, total), key index = row * C + class): count, box / score / class / row
// per detection, and the optional lists.  flag[NMS_KEPT_MAX] and wsum are scratch.
__device__ __forceinline__ void det_write_outputs(const u64* kept_key, int total, int C, const float* cbx, const ScanOut& o, int* flag,
                                                  int* wsum) {
  const int tid = threadIdx.x;
  if (total > o.cap) total = o.cap;
  if (total > NMS_KEPT_MAX) total = NMS_KEPT_MAX;
  if (tid == 0 && o.out_count) *o.out_count = total;
  int my_row = -1;
  if (tid < total) {
    const u64 k = kept_key[tid];
    const int slot = (int)key_index(k);
    int r = slot / C;
    const int cl = slot - r * C;
    r = r < 0 ? 0 : (r >= DET_MAX_R ? DET_MAX_R - 1 : r);
    my_row = r;
    if (o.out_boxes) {
      o.out_boxes[tid * 4 + 0] = cbx[r * 4 + 0];
      o.out_boxes[tid * 4 + 1] = cbx[r * 4 + 1];
      o.out_boxes[tid * 4 + 2] = cbx[r * 4 + 2];
      o.out_boxes[tid * 4 + 3] = cbx[r * 4 + 3];
    }
    if (o.out_scores) o.out_scores[tid] = key_score(k);
    if (o.out_labels) o.out_labels[tid] = cl;
    if (o.out_rows) o.out_rows[tid] = r;
  }
  const bool row_flagged = tid < total && my_row >= 0 && my_row < NMS_KEPT_MAX;
  if (o.rep_of) {
    // entries of one source row carry the same box: the first of them represents the group (the mask head is class agnostic)
    if (tid < NMS_KEPT_MAX) flag[tid] = 0x7FFFFFFF;
    __syncthreads();
    if (row_flagged) atomicMin(&flag[my_row], tid);
    __syncthreads();
    bool is_rep = false;
    if (tid < total) {
      const int rep = row_flagged ? flag[my_row] : tid;
      o.rep_of[tid] = rep;
      is_rep = rep == tid;
    }
    int all;
    const int pos = block_compact_flags(is_rep, wsum, &all);
    if (tid < NMS_KEPT_MAX && is_rep) o.rep_list[pos] = tid;
    if (tid == 0) *o.rep_count = all;
    __syncthreads();
  }
  if (o.uniq_rows) {
    // torch.unique of the kept rows: flags over the row ids (< NMS_KEPT_MAX), ballot compaction, ascending
    if (tid < NMS_KEPT_MAX) flag[tid] = 0;
    __syncthreads();
    if (row_flagged) flag[my_row] = 1;
    __syncthreads();
    const bool f = tid < NMS_KEPT_MAX && flag[tid] != 0;
    int all;
    const int pos = block_compact_flags(f, wsum, &all);
    if (f && pos < o.uniq_cap) o.uniq_rows[pos] = tid;
    if (tid == 0 && o.uniq_count) *o.uniq_count = all < o.uniq_cap ? all : o.uniq_cap;
  }
}

// det_row_iou_matrix as a launch of its own: the same bit matrix into a caller-owned [R_cap, words] array (words = ceil(R_cap / 64):
// every word is written, zero beyond the rows in use), from the same clipped boxes and the same comparison, so that a selection that is
// handed the matrix (EodDetDesc.row_matrix) keeps the same detections.  The matrix needs the boxes only, not the scores: it can be
// built while the launches that produce the scores still run.  Workgroup (w, t, scene): the 64 rows of tile t against the 64 partner
// rows of word w; four neighbouring lanes take 16 partners each of one row and OR their bits together.
__global__ __launch_bounds__(256) void det_row_matrix_kernel(const float* __restrict__ boxes, const int* __restrict__ count, int R_cap,
                                                               int words, float img_w, float img_h, float nms_thresh,
                                                               u64* __restrict__ out) {
  const int scene = blockIdx.z;
  boxes += (size_t)scene * R_cap * 4;
  out += (size_t)scene * R_cap * words;
  __shared__ float rowb[64 * 4];      // the tile's rows, clipped
  __shared__ float parb[64 * 4];      // the word's partner rows, clipped
  int R = R_cap;
  if (count) {
    const int c = count[scene];
    R = c < R ? c : R;
  }
  const int tid = threadIdx.x, w = blockIdx.x, r0 = blockIdx.y * 64;
  if (tid < 64) {
    det_clip_row(boxes + (size_t)r0 * 4, tid, r0 + tid < R, img_w, img_h, rowb);
  } else if (tid < 128) {
    const int b = tid - 64;
    det_clip_row(boxes + (size_t)w * 64 * 4, b, w * 64 + b < R, img_w, img_h, parb);
  }
  __syncthreads();
  const int lr = tid >> 2, quarter = tid & 3, r = r0 + lr;
  u64 bits = 0;
  if (r < R) {
    const float x1 = rowb[lr * 4 + 0], y1 = rowb[lr * 4 + 1], x2 = rowb[lr * 4 + 2], y2 = rowb[lr * 4 + 3];
    const float area = (x2 - x1) * (y2 - y1);
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
      const int b = quarter * 16 + k, r2 = w * 64 + b;
      if (r2 < R && r2 != r && iou_over(x1, y1, x2, y2, area, parb[b * 4 + 0], parb[b * 4 + 1], parb[b * 4 + 2], parb[b * 4 + 3], nms_thresh))
        bits |= 1ull << b;
    }
  }
  bits |= __shfl_xor(bits, 1, 64);
  bits |= __shfl_xor(bits, 2, 64);
  if (quarter == 0 && r < R_cap) out[(size_t)r * words + w] = bits;
}

__global__ __launch_bounds__(1024) void det_select_kernel(const float* boxes, const float* scores, const int* count, int R_cap, int C1,
                                                           float img_w, float img_h, float thr, float nms_thresh, int topk, ScanOut o,
                                                           const u64* __restrict__ row_matrix) {
  EOD_CHAIN_PRIO();
  constexpr int EMAX = 8;
  {
    const int scene = blockIdx.x;      // one workgroup per scene of a batch
    if (row_matrix) row_matrix += (size_t)scene * R_cap * ((R_cap + 63) >> 6);
    boxes += (size_t)scene * R_cap * 4;
    scores += (size_t)scene * R_cap * C1;
    if (count) count += scene;
    o = scene_outputs(o, scene);
  }
  __shared__ u64 buf[1024 * EMAX];                 // compaction target / sort exchange / sorted keys of the batch
  __shared__ u64 Mx[DET_MAX_R * DET_WORDS];        // IoU bit matrix of the rows
  __shared__ float cbx[DET_MAX_R * 4];             // clipped boxes
  __shared__ u64 supp[DET_MAX_C * DET_WORDS];      // per class: rows suppressed by the kept detections of that class
  __shared__ int hist[4096];
  __shared__ u64 kept_key[NMS_KEPT_MAX];
  __shared__ int flag[NMS_KEPT_MAX];
  __shared__ int wsum[16];
  __shared__ u64 keptbits[1024 * 8 / 64];          // bit q: entry q of the sorted batch survives its class's NMS
  __shared__ int wordpre[128];
  __shared__ unsigned char row_ok[DET_MAX_R];
  __shared__ int sh_cnt, sh_cut, sh_n2, sh_total, sh_done;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int R = R_cap;
  if (count) {
    const int c = *count;
    R = c < R ? c : R;
  }
  const int C = C1 - 1;
  const int slots = R_cap * C;
  const int W = (R + 63) >> 6;
#ifdef EOD_STAMPS
  const int sb = topk <= 100 ? 8 : 24;
#endif
  EOD_STAMP(sb + 0);
  for (int i = tid; i < 4096; i += 1024) hist[i] = 0;
  for (int i = tid; i < DET_MAX_C * DET_WORDS; i += 1024) supp[i] = 0;
  if (tid == 0) {
    sh_cnt = 0;
    sh_cut = 0;
    sh_n2 = 0;
    sh_total = 0;
    sh_done = 0;
  }
  // a row takes part only if its box and ALL its scores are finite (d2 fast_rcnn_inference drops the others)
  for (int r = tid; r < R_cap; r += 1024) {
    bool fin = det_clip_row(boxes, r, r < R, img_w, img_h, cbx);
    if (r < R)
      for (int q = 0; q < C1; ++q) fin = fin & (bool)isfinite(scores[r * C1 + q]);
    row_ok[r] = fin ? 1 : 0;
  }
  // the thread's scores: eight independent loads, one latency (slot i = e * 1024 + tid = (row, class))
  float sc[EMAX];
#pragma unroll
  for (int e = 0; e < EMAX; ++e) {
    const int i = e * 1024 + tid;
    const int r = i / C, c = i - r * C;
    sc[e] = (i < slots && r < R) ? scores[r * C1 + c] : -1.0f;
  }
  __syncthreads();
  EOD_STAMP(sb + 1);
  if (row_matrix) {
    // built ahead by det_row_matrix_kernel from these boxes, this size and this threshold: the words that are read
    const int words = (R_cap + 63) >> 6;
    for (int idx = tid; idx < R * W; idx += 1024) {
      const int r = idx / W, w = idx - r * W;
      Mx[r * DET_WORDS + w] = row_matrix[(size_t)r * words + w];
    }
  } else {
    det_row_iou_matrix(cbx, R, W, nms_thresh, Mx);
  }
  EOD_STAMP(sb + 2);
  // candidates: score > thr on a finite row; histogram of their score bits
  u64 key[EMAX];
  int local = 0;
#pragma unroll
  for (int e = 0; e < EMAX; ++e) {
    const int i = e * 1024 + tid;
    u64 k = 0;
    if (i < slots && row_ok[i / C] && sc[e] > thr) {
      k = make_key(sc[e], (unsigned)i);
      atomicAdd(&hist[score_bin(__float_as_uint(sc[e]))], 1);
      ++local;
    }
    key[e] = k;
  }
  if (local) atomicAdd(&sh_cnt, local);
  __syncthreads();
  const int n = sh_cnt;
  // the lowest bin whose suffix holds min(n, 1024) candidates
  const int cut = block_hist_cut(hist, n < 1024 ? n : 1024, wsum, &sh_cut);
  EOD_STAMP(sb + 3);
  for (int batch = 0; batch < 2; ++batch) {
    // batch 0: the candidates of the bins >= cut; batch 1 (only if batch 0 did not fill the list): all the others
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
      const bool hi = score_bin((unsigned)(key[e] >> 32)) >= cut;
      wave_compact_key(key[e] != 0 && (batch == 0 ? hi : !hi), key[e], &sh_n2, buf);
    }
    __syncthreads();
    const int n2 = sh_n2;
    block_sort_keys<EMAX>(buf, n2);
    EOD_STAMP(sb + 4 + 2 * batch);
    // Greedy NMS over the sorted batch, per class and in parallel: suppression only acts inside a class, so the greedy walk over
    // the whole list is the same as C independent walks over each class's entries in list order.  Wave w takes classes w, w + 16:
    // per 64-entry chunk one ballot finds its class's entries (a few per chunk), each is a bit test against the class's suppressed-
    // row set and, if kept, an OR of its row of the IoU matrix into that set (LDS, in program order within the wave).  (First
    // version: ONE wave walked all entries of all classes, 128 dependent shuffle steps per chunk: 45 us to keep 100, 131 us to keep
    // 300.)  The kept entries are then ranked in list order and the first (topk - total) of them taken.
    for (int i = tid; i < 1024 * EMAX / 64; i += 1024) keptbits[i] = 0;
    __syncthreads();
    for (int cls = wave; cls < C; cls += 16) {
      // the class's suppressed-row set lives in registers for the walk: lane w holds word w
      u64 myw = lane < DET_WORDS ? supp[cls * DET_WORDS + lane] : 0ull;
      for (int c0 = 0; c0 < n2; c0 += 64) {
        const int q = c0 + lane;
        int r = 0, mycl = -1;
        if (q < n2) {
          const int slot = (int)key_index(buf[q]);
          r = slot / C;
          mycl = slot - r * C;
        }
        u64 m = __ballot(mycl == cls);
        u64 keptmask = 0;
        while (m) {
          const int j = (int)__ffsll((long long)m) - 1;
          m &= m - 1;
          // j and rj are wave-uniform (they come from the ballot): v_readlane into scalar registers, no LDS-crossbar shuffle
          const int rj = __builtin_amdgcn_readlane(r, j);
          const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(myw & 0xFFFFFFFFull), rj >> 6);
          const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(myw >> 32), rj >> 6);
          const u64 word = ((u64)hi << 32) | lo;
          if (!((word >> (rj & 63)) & 1ull)) {               // wave-uniform
            keptmask |= 1ull << j;
            if (lane < W) myw |= Mx[rj * DET_WORDS + lane];
          }
        }
        if (lane == 0 && keptmask) atomicOr(&keptbits[c0 >> 6], keptmask);
      }
      if (lane < DET_WORDS) supp[cls * DET_WORDS + lane] = myw;
    }
    __syncthreads();
    // the kept entries are ranked in list order and the first (topk - total) of them taken
    const int total0 = sh_total;
    const int kept_all = block_rank_and_take<1024 * EMAX / 64>(keptbits, n2, total0, topk, buf, kept_key, wordpre, wsum);
    __syncthreads();
    if (tid == 0) {
      int total = total0 + kept_all;
      const bool full = total >= topk;
      if (full) total = topk;
      sh_total = total;
      // done when the list is full or no candidate is left for a second batch
      sh_done = (full || batch == 1 || n2 >= n) ? 1 : 0;
      sh_n2 = 0;
    }
    __syncthreads();
    EOD_STAMP(sb + 5 + 2 * batch);
    if (sh_done) break;
  }
  __syncthreads();
  det_write_outputs(kept_key, sh_total, C, cbx, o, flag, wsum);
  EOD_STAMP(sb + 8);
#ifdef EOD_STAMPS
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    eod_stamps[sb + 9] = (unsigned long long)sh_cnt;       // candidates above the threshold
    eod_stamps[sb + 10] = (unsigned long long)sh_total;    // kept
  }
#endif
}

// The scene-local index lists of a batch (kept proposal rows, detection-group representatives) as ONE list of global indices
// b * id_stride + list[b][k], scene by scene: the mask head then runs once over the concatenation with a single count.
__global__ __launch_bounds__(256) void concat_lists_kernel(const int* __restrict__ lists, const int* __restrict__ counts, int cap_in,
                                                            int id_stride, int batch, int* __restrict__ out, int* __restrict__ out_count) {
  EOD_CHAIN_PRIO();
  int off = 0;
  for (int b = 0; b < batch; ++b) {
    int c = counts[b];
    c = c < 0 ? 0 : (c > cap_in ? cap_in : c);
    for (int k = threadIdx.x; k < c; k += blockDim.x) out[off + k] = b * id_stride + lists[(size_t)b * cap_in + k];
    off += c;
  }
  if (threadIdx.x == 0) *out_count = off;
}

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------------
// fast_rcnn_inference for wide vocabularies (more than DET_MAX_C classes or more than 8192 slots): three launches
// ------------------------------------------------------------------------------------------------------
// The [R, C1] score matrix (LVIS: 256 x 1204) no longer fits one workgroup's registers and C suppressed-row sets no longer fit
// LDS.  The pieces of det_select_kernel carry over -- 64-bit (score, slot) keys, the histogram cut on the score bits, the in-LDS
// sort, the R x R row-IoU bit matrix that turns per-class NMS into bit tests -- in this shape:
//   (a) detw_hist_kernel, two rows per workgroup over the whole chip: finite-row flags, threshold, the scene's histogram of the
//       candidates' score bins (workspace), and the scene's suppressed-row sets cleared;
//   (b) detw_compact_kernel, same grid: every workgroup derives the same cut from the histogram -- the lowest bin whose suffix
//       holds at most DETW_BATCH candidates -- and appends its rows' keys of the bins above the cut to the scene's list;
//   (c) detw_tail_kernel, one workgroup per scene: sorts the list (a prefix of the fully sorted candidates), runs the per-class greedy
//       NMS on it, ranks the kept entries and takes the first topk.  If the list is not full and candidates are left it fetches the
//       NEXT DETW_BATCH keys below the last one itself -- a radix select over the 64-bit keys by re-scanning the score matrix, up to
//       six histogram scans and one collecting scan: slow, rare, and exactly the greedy NMS over the fully sorted list -- and goes
//       on, with the suppressed-row sets of the classes kept in the workspace between batches.
// The hand-over between (a), (b) and (c) is the kernel boundary.  (c) leaves the histogram and the list's counter zeroed: the
// workspace has to be zero before the first call only (ops.DetectionSelector allocates it so); no memset per call.
// NMS inside a batch: a second sort by (class, position in the batch) makes every class's entries a contiguous run in score order;
// one LANE per run walks it with the class's suppressed-row set in 8 registers (test bit r, OR row r of the IoU matrix when kept).
#define DETW_MAX_C 2047
#define DETW_BATCH 4096            // keys per sorted batch
#define DETW_WANT 2048             // the first cut aims at this many candidates (and takes up to DETW_BATCH)

struct DetwWs {
  int* hist;           // [nb][4096]
  int* cand_cnt;       // [nb]
  unsigned char* row_ok;   // [nb][DET_MAX_R]
  u64* cand;           // [nb][DETW_BATCH]
  u64* supp;           // [nb][C][DET_WORDS]
  size_t bytes;
};

DetwWs carve_detw(void* base, int C, int nb) {
  DetwWs w{};
  size_t off = 0;
  char* b = static_cast<char*>(base);
  auto take = [&](size_t bytes) {
    char* p = b ? b + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  w.hist = reinterpret_cast<int*>(take((size_t)nb * 4096 * sizeof(int)));
  w.cand_cnt = reinterpret_cast<int*>(take((size_t)EOD_MAX_BATCH * sizeof(int)));
  w.row_ok = reinterpret_cast<unsigned char*>(take((size_t)nb * DET_MAX_R));
  w.cand = reinterpret_cast<u64*>(take((size_t)nb * DETW_BATCH * sizeof(u64)));
  w.supp = reinterpret_cast<u64*>(take((size_t)nb * C * DET_WORDS * sizeof(u64)));
  w.bytes = off;
  return w;
}

__device__ __forceinline__ int detw_rows(const int* count, int scene, int R_cap) {
  int R = R_cap;
  if (count) {
    const int c = count[scene];
    R = c < R ? (c < 0 ? 0 : c) : R;
  }
  return R;
}

// (a): grid (ceil(R_cap / 2), scenes), 256 threads; a thread holds up to 8 scores of the workgroup's current row
__global__ __launch_bounds__(256) void detw_hist_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                         const int* __restrict__ count, int R_cap, int C1, float thr, DetwWs ws) {
  EOD_CHAIN_PRIO();
  const int scene = blockIdx.y, tid = threadIdx.x;
  const int C = C1 - 1;
  const int R = detw_rows(count, scene, R_cap);
  boxes += (size_t)scene * R_cap * 4;
  scores += (size_t)scene * R_cap * C1;
  // this workgroup's share of the scene's suppressed-row sets (read by (c) only when a selection needs a second batch)
  {
    u64* supp = ws.supp + (size_t)scene * C * DET_WORDS;
    const int n = C * DET_WORDS;
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) supp[i] = 0ull;
  }
  __shared__ int sh_fin;
  for (int rr = 0; rr < 2; ++rr) {
    const int r = blockIdx.x * 2 + rr;
    if (r >= R_cap) break;                                   // workgroup-uniform
    if (tid == 0) sh_fin = 1;
    __syncthreads();
    float sc[8];
    bool fin = true;
    if (r < R) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = tid + 256 * e;
        sc[e] = c < C1 ? scores[(size_t)r * C1 + c] : 0.f;
        fin = fin & (bool)isfinite(sc[e]);
      }
      if (tid < 4) fin = fin & (bool)isfinite(boxes[r * 4 + tid]);
    } else {
      fin = false;
#pragma unroll
      for (int e = 0; e < 8; ++e) sc[e] = 0.f;
    }
    if (!fin) sh_fin = 0;
    __syncthreads();
    const bool ok = sh_fin != 0;                             // the box and ALL scores of the row are finite
    if (tid == 0) ws.row_ok[(size_t)scene * DET_MAX_R + r] = ok ? 1 : 0;
    if (ok) {
      int* hist = ws.hist + (size_t)scene * 4096;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = tid + 256 * e;
        if (c < C && sc[e] > thr) atomicAdd(&hist[score_bin(__float_as_uint(sc[e]))], 1);
      }
    }
    __syncthreads();
  }
}

// the cut of a scene: the lowest bin whose suffix holds at most DETW_BATCH candidates, going down until DETW_WANT are covered.
// 256 threads, 16 bins each; every workgroup of (b) and the tail workgroup compute the same value from the same histogram.
// Returns the cut (0..4096; 4096 = no bin fits) and the scene's candidate count through *total.
__device__ __forceinline__ int detw_cut(const int* __restrict__ hist, int* sh_wsum /*[4]*/, int* sh_out /*[1]*/, int* total) {
  const int tid = threadIdx.x;
  int h[16];
  if (tid < 256) {
#pragma unroll
    for (int j = 0; j < 16; ++j) h[j] = hist[tid * 16 + j];
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) h[j] = 0;
  }
  if (tid == 0) *sh_out = 4096;
  int suf = block_bins_above<16>(h, sh_wsum);                // candidates in the bins above this thread's
  *total = sh_wsum[0] + sh_wsum[1] + sh_wsum[2] + sh_wsum[3];
  if (tid < 256) {
    // suffix counts of this thread's bins; a bin b is "takeable" iff suffix(b) <= DETW_BATCH; the cut is the lowest takeable bin
    // that is still needed: suffix(b + 1) < DETW_WANT
    int best = 4096;
#pragma unroll
    for (int j = 15; j >= 0; --j) {
      const int above = suf;
      suf += h[j];
      if (suf <= DETW_BATCH && above < DETW_WANT && h[j] > 0) best = tid * 16 + j;
    }
    if (best < 4096) atomicMin(sh_out, best);
  }
  __syncthreads();
  return *sh_out;
}

// (b): same grid as (a)
__global__ __launch_bounds__(256) void detw_compact_kernel(const float* __restrict__ scores, const int* __restrict__ count, int R_cap,
                                                            int C1, float thr, DetwWs ws) {
  EOD_CHAIN_PRIO();
  const int scene = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int C = C1 - 1;
  __shared__ int sh_wsum[4], sh_out;
  int total;
  const int cut = detw_cut(ws.hist + (size_t)scene * 4096, sh_wsum, &sh_out, &total);
  if (cut >= 4096) return;                                   // nothing to take on the fast path
  scores += (size_t)scene * R_cap * C1;
  u64* cand = ws.cand + (size_t)scene * DETW_BATCH;
  for (int rr = 0; rr < 2; ++rr) {
    const int r = blockIdx.x * 2 + rr;
    if (r >= R_cap || !ws.row_ok[(size_t)scene * DET_MAX_R + r]) continue;      // workgroup-uniform
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = tid + 256 * e;
      float v = -1.f;
      if (c < C) v = scores[(size_t)r * C1 + c];
      const bool in = c < C && v > thr && score_bin(__float_as_uint(v)) >= cut;
      const u64 bal = __ballot(in);
      if (!bal) continue;
      int base = 0;
      if (lane == 0) base = atomicAdd(&ws.cand_cnt[scene], __popcll(bal));
      base = __shfl(base, 0, 64);
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      if (in && pos >= 0 && pos < DETW_BATCH) cand[pos] = make_key(v, (unsigned)(r * C + c));
    }
  }
}

// One scan of the scene's score matrix by the tail workgroup: calls f(key) for every candidate (finite row, score > thr).
template <typename F>
__device__ __forceinline__ void detw_scan(const float* __restrict__ scores, const unsigned char* row_ok, int R, int C, int C1, float thr, F f) {
  for (int r = 0; r < R; ++r) {
    if (!row_ok[r]) continue;
    for (int c = threadIdx.x; c < C; c += 1024) {
      const float v = scores[(size_t)r * C1 + c];
      if (v > thr) f(make_key(v, (unsigned)(r * C + c)));
    }
  }
}

// (c): one workgroup per scene
__global__ __launch_bounds__(1024) void detw_tail_kernel(const float* boxes, const float* scores, const int* count, int R_cap, int C1,
                                                          float img_w, float img_h, float thr, float nms_thresh, int topk, DetwWs ws,
                                                          ScanOut o) {
  EOD_CHAIN_PRIO();
  const int scene = blockIdx.x;
  boxes += (size_t)scene * R_cap * 4;
  scores += (size_t)scene * R_cap * C1;
  o = scene_outputs(o, scene);
  int* g_hist = ws.hist + (size_t)scene * 4096;
  const u64* g_cand = ws.cand + (size_t)scene * DETW_BATCH;
  const int C = C1 - 1;
  u64* g_supp = ws.supp + (size_t)scene * C * DET_WORDS;
  __shared__ u64 buf[DETW_BATCH];                  // the batch's keys, sorted descending
  __shared__ u64 comp[DETW_BATCH];                 // the batch's entries ordered by (class, position)
  __shared__ u64 Mx[DET_MAX_R * DET_WORDS];        // IoU bit matrix of the rows
  __shared__ float cbx[DET_MAX_R * 4];             // clipped boxes
  __shared__ int hist[4096];
  __shared__ int segstart[DETW_MAX_C + 1];
  __shared__ u64 kept_key[NMS_KEPT_MAX];
  __shared__ int flag[NMS_KEPT_MAX];
  __shared__ u64 keptbits[DETW_BATCH / 64];
  __shared__ int wordpre[DETW_BATCH / 64];
  __shared__ int wsum[16];
  __shared__ unsigned char row_ok[DET_MAX_R];
  __shared__ int sh_wsum[4], sh_out, sh_n2, sh_nseg, sh_total, sh_done;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = detw_rows(count, scene, R_cap);
  const int W = (R + 63) >> 6;
  int n_all;
  const int cut = detw_cut(g_hist, sh_wsum, &sh_out, &n_all);
  (void)cut;
  __syncthreads();
  // the list (b) left, and the workspace as the next call expects it
  int n2 = ws.cand_cnt[scene];
  n2 = n2 < 0 ? 0 : (n2 > DETW_BATCH ? DETW_BATCH : n2);
  for (int i = tid; i < n2; i += 1024) buf[i] = g_cand[i];
  for (int i = tid; i < 4096; i += 1024) g_hist[i] = 0;
  for (int r = tid; r < DET_MAX_R; r += 1024) {
    const bool in = r < R;
    row_ok[r] = in ? ws.row_ok[(size_t)scene * DET_MAX_R + r] : 0;
    det_clip_row(boxes, r, in, img_w, img_h, cbx);
  }
  if (tid == 0) {
    sh_total = 0;
    sh_done = 0;
  }
  __syncthreads();
  if (tid == 0) ws.cand_cnt[scene] = 0;
  det_row_iou_matrix(cbx, R, DET_WORDS, nms_thresh, Mx);     // all words of a row are written
  __syncthreads();
  int processed = 0;                 // candidates of the batches walked so far
  u64 bound = ~0ull;                 // every key of the batches walked so far is >= bound; the next batch lies below it
  for (int round = 0;; ++round) {
    if (round > 0 || n2 == 0) {
      // ---- the next DETW_BATCH keys below `bound`: radix select by re-scanning the score matrix
      if (processed >= n_all) break;                         // uniform
      u64 lo = 0;                    // the interval searched is [lo, lo + 2^(s + w)), below `bound`
      int acc = 0;                   // keys accepted so far: those of the interval's upper neighbours below `bound`
      u64 T = 0;
      int sft = 52, wid = 12;
      for (int level = 0; level < 6; ++level) {
        for (int i = tid; i < 4096; i += 1024) hist[i] = 0;
        __syncthreads();
        const int top = sft + wid;
        detw_scan(scores, row_ok, R, C, C1, thr, [=](u64 k) {
          if (k < bound && (top >= 64 || (k >> top) == (lo >> top))) atomicAdd(&hist[(int)((k >> sft) & ((1u << wid) - 1u))], 1);
        });
        __syncthreads();
        // the smallest digit d with acc + suffix(d) <= DETW_BATCH (4096 = none of this interval)
        if (tid == 0) sh_out = 4096;
        int h4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h4[j] = hist[tid * 4 + j];
        int suf = block_bins_above<4>(h4, wsum);
        int best = 4096;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
          suf += h4[j];
          if (acc + suf <= DETW_BATCH) best = tid * 4 + j;
        }
        if (best < 4096) atomicMin(&sh_out, best);
        __syncthreads();
        const int d = sh_out;
        // suffix(d): every thread sums the bins it owns that are >= d, then the workgroup total
        int part = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (tid * 4 + j >= d) part += h4[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        __syncthreads();
        if (lane == 0) wsum[wave] = part;
        __syncthreads();
        int sufd = 0;
        for (int w = 0; w < 16; ++w) sufd += wsum[w];
        __syncthreads();
        acc += sufd;
        T = (d >= 4096 && top >= 64) ? ~0ull : lo + ((u64)d << sft);        // (no bin of the whole key range fits: nothing)
        if (d == 0 || acc >= 1024 || sft == 0) break;        // uniform
        lo += (u64)(d - 1) << sft;                           // descend into the bin that did not fit as a whole
        if (sft >= 16) {
          sft -= 12;
        } else {
          sft = 0;
          wid = 4;
        }
      }
      // collect T <= key < bound
      if (tid == 0) sh_n2 = 0;
      __syncthreads();
      detw_scan(scores, row_ok, R, C, C1, thr, [=](u64 k) {
        if (k < bound && k >= T) {
          const int pos = atomicAdd(&sh_n2, 1);
          if (pos < DETW_BATCH) buf[pos] = k;
        }
      });
      __syncthreads();
      n2 = sh_n2 < DETW_BATCH ? sh_n2 : DETW_BATCH;
      __syncthreads();
      if (n2 == 0) break;                                    // cannot happen while candidates are left; never spin
    }
    block_sort_keys<4>(buf, n2);
    // ---- entries by (class ascending, position ascending): descending sort of ((2047 - class) << 16 | (0xFFFF - position))
    for (int q = tid; q < n2; q += 1024) {
      const int slot = (int)key_index(buf[q]);
      const int r = slot / C, cl = slot - r * C;
      comp[q] = ((u64)(2047 - cl) << 16) | (u64)(0xFFFF - q);
    }
    for (int i = tid; i < DETW_BATCH / 64; i += 1024) keptbits[i] = 0;
    if (tid == 0) sh_nseg = 0;
    __syncthreads();
    block_sort_keys<4>(comp, n2);
    for (int q = tid; q < n2; q += 1024) {
      if (q == 0 || (comp[q] >> 16) != (comp[q - 1] >> 16)) {
        const int pos = atomicAdd(&sh_nseg, 1);
        if (pos <= DETW_MAX_C) segstart[pos] = q;
      }
    }
    __syncthreads();
    const int nseg = sh_nseg <= DETW_MAX_C ? sh_nseg : DETW_MAX_C;
    // ---- per-class greedy NMS: one lane per class run (the order of the runs does not matter, classes are independent)
    for (int sgi = tid; sgi < nseg; sgi += 1024) {
      const int q0 = segstart[sgi];
      const u64 ctag = comp[q0] >> 16;
      int cl = 2047 - (int)ctag;
      cl = cl < 0 ? 0 : (cl >= C ? C - 1 : cl);
      u64 w[DET_WORDS];
#pragma unroll
      for (int j = 0; j < DET_WORDS; ++j) w[j] = g_supp[(size_t)cl * DET_WORDS + j];         // cleared by (a), carried from batch to batch
      for (int p = q0; p < n2; ++p) {
        const u64 ce = comp[p];
        if ((ce >> 16) != ctag) break;
        int q = 0xFFFF - (int)(ce & 0xFFFFull);
        q = q < 0 ? 0 : (q >= n2 ? n2 - 1 : q);
        int r = (int)key_index(buf[q]) / C;
        r = r < 0 ? 0 : (r >= DET_MAX_R ? DET_MAX_R - 1 : r);
        u64 word = 0;
#pragma unroll
        for (int j = 0; j < DET_WORDS; ++j) word = (j == (r >> 6)) ? w[j] : word;
        if (!((word >> (r & 63)) & 1ull)) {
          atomicOr(&keptbits[q >> 6], 1ull << (q & 63));
#pragma unroll
          for (int j = 0; j < DET_WORDS; ++j)
            if (j < W) w[j] |= Mx[r * DET_WORDS + j];       // (the words beyond W are zero; the guard keeps the loads few)
        }
      }
#pragma unroll
      for (int j = 0; j < DET_WORDS; ++j) g_supp[(size_t)cl * DET_WORDS + j] = w[j];
    }
    __syncthreads();
    // ---- rank of every kept entry in list order; the first (topk - total) of them are taken
    const int total0 = sh_total;
    const int kept_all = block_rank_and_take<DETW_BATCH / 64>(keptbits, n2, total0, topk, buf, kept_key, wordpre, wsum);
    __syncthreads();
    if (tid == 0) {
      int total = total0 + kept_all;
      const bool full = total >= topk;
      if (full) total = topk;
      sh_total = total;
      sh_done = (full || processed + n2 >= n_all) ? 1 : 0;
    }
    const u64 last = buf[n2 - 1];
    __syncthreads();
    if (sh_done) break;
    processed += n2;
    bound = last;
  }
  __syncthreads();
  det_write_outputs(kept_key, sh_total, C, cbx, o, flag, wsum);
}


struct SelWs {
  float* sorted_boxes;
  float* sorted_scores;
  int* sorted_labels;   // (these two lists are not in use; they stay in the layout, and so in the workspace sizes the library reports)
  int* sorted_rows;
  u64* cand_keys;
  int* cand_cnt;
  size_t bytes;
};

SelWs carve(void* base, int cap_sort, int keep_cap, int cand_slots) {
  SelWs w{};
  size_t off = 0;
  char* b = static_cast<char*>(base);
  (void)keep_cap;
  auto take = [&](size_t bytes) {
    char* p = b ? b + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  w.sorted_boxes = reinterpret_cast<float*>(take((size_t)cap_sort * 4 * sizeof(float)));
  w.sorted_scores = reinterpret_cast<float*>(take((size_t)cap_sort * sizeof(float)));
  w.sorted_labels = reinterpret_cast<int*>(take((size_t)cap_sort * sizeof(int)));
  w.sorted_rows = reinterpret_cast<int*>(take((size_t)cap_sort * sizeof(int)));
  w.cand_keys = reinterpret_cast<u64*>(take((size_t)(cand_slots > 0 ? cand_slots : 1) * sizeof(u64)));
  w.cand_cnt = reinterpret_cast<int*>(take(8 * EOD_MAX_BATCH * sizeof(int)));
  w.bytes = off;
  return w;
}

}  // namespace

// Wide lists (levels * pre_nms_topk > 8192, the training thresholds): the packed candidate slots are bounded by the pyramid's
// positions; behind the narrow layout sit the candidate count per scene and the suppression bit matrix.
struct WideWs {
  int slots;       // bound of the packed candidate slots of one scene
  int words;       // 64-bit words per matrix row
  int* n;          // [batch]
  u64* matrix;     // [batch][slots][words]
  size_t bytes;
};

static WideWs carve_wide(void* base, size_t narrow_bytes, int total_positions, int levels, int pre_nms_topk, int nb) {
  WideWs w{};
  w.slots = std::min(total_positions, levels * pre_nms_topk);
  w.words = (w.slots + 63) / 64;
  char* b = static_cast<char*>(base);
  size_t off = narrow_bytes;
  w.n = reinterpret_cast<int*>(b ? b + off : nullptr);
  off += align_up(EOD_MAX_BATCH * sizeof(int));
  w.matrix = reinterpret_cast<u64*>(b ? b + off : nullptr);
  off += align_up((size_t)nb * w.slots * w.words * sizeof(u64));
  w.bytes = off;
  return w;
}

extern "C" size_t eod_proposals_workspace_bytes(int total_positions, int levels, int pre_nms_topk, int batch) {
  const int slots = levels * pre_nms_topk, nb = batch > 1 ? batch : 1;
  if (slots > 8192) {
    const int ws = std::max(std::min(total_positions, slots), 1);
    const size_t narrow = carve(nullptr, ws * nb, ws, ws * nb).bytes;
    return carve_wide(nullptr, narrow, total_positions, levels, pre_nms_topk, nb).bytes;
  }
  return carve(nullptr, slots * nb, slots, slots * nb).bytes;
}

// What both proposal paths do first: the level sizes are validated and the kernels' argument struct filled from the descriptor, all
// but the candidate lists (they follow the path's workspace layout).  The per-level candidate lists are packed: level l holds at
// most min(level size, topk) entries, pk_off[levels] is the packed slot count of a scene.
static int cn_args(const EodProposalDesc* d, int nb, CnArgs* a) {
  a->batch = nb;
  a->head = d->head_out; a->head_stride = d->head_stride; a->levels = d->levels;
  a->score_thresh = d->score_thresh; a->topk = d->pre_nms_topk;
  a->pk_off[0] = 0;
  for (int l = 0; l < d->levels; ++l) {
    const int n = d->level_off[l + 1] - d->level_off[l];
    if (n <= 0 || n > EOD_SORT_MAX || d->level_w[l] <= 0 || n % d->level_w[l] != 0) return EOD_ERR_CAPACITY;
    a->level_off[l] = d->level_off[l];
    a->level_w[l] = d->level_w[l];
    a->level_stride[l] = d->level_stride[l];
    a->level_scale[l] = d->level_scale[l];
    a->pk_off[l + 1] = a->pk_off[l] + std::min(n, d->pre_nms_topk);
  }
  a->level_off[d->levels] = d->level_off[d->levels];
  return EOD_OK;
}

// per-level top-k into the lists of `w`: one workgroup per level and scene, sized by the largest level
static void cn_launch_level_topk(CnArgs* a, const SelWs& w, hipStream_t s) {
  a->cand_keys = w.cand_keys; a->cand_cnt = w.cand_cnt;
  int max_level = 0;
  for (int l = 0; l < a->levels; ++l) max_level = std::max(max_level, a->level_off[l + 1] - a->level_off[l]);
  if (max_level <= 8192)
    hipLaunchKernelGGL(cn_level_topk_kernel<8>, dim3(a->levels, a->batch), dim3(1024), 0, s, *a);
  else
    hipLaunchKernelGGL(cn_level_topk_kernel<16>, dim3(a->levels, a->batch), dim3(1024), 0, s, *a);
}

// centernet.py:603-745 with lists beyond one workgroup's LDS (see the kernels above)
static int centernet_proposals_wide(const EodProposalDesc* d, hipStream_t s) {
  const int total = d->level_off[d->levels];
  const int nb = d->batch > 1 ? d->batch : 1;
  CnArgs a{};
  if (const int err = cn_args(d, nb, &a)) return err;
  const int packed = a.pk_off[d->levels];
  if (packed > WIDE_MAX_SLOTS || d->cap < d->post_nms_topk || d->cap > WIDE_MAX_CAP) return EOD_ERR_CAPACITY;
  if (nb > EOD_MAX_BATCH) return EOD_ERR_BAD_DIMS;
  const int ws = std::min(total, d->levels * d->pre_nms_topk);          // >= packed
  const SelWs w = carve(d->workspace, ws * nb, ws, ws * nb);
  const WideWs ww = carve_wide(d->workspace, w.bytes, total, d->levels, d->pre_nms_topk, nb);
  if (d->workspace_bytes < ww.bytes) return EOD_ERR_CAPACITY;
  cn_launch_level_topk(&a, w, s);
  // the kernels below address the scenes' lists with the PACKED slot count as their stride
  const int words = (packed + 63) / 64;
  hipLaunchKernelGGL(cn_rank_decode_kernel, dim3((packed + 255) / 256, nb), dim3(256), 0, s, a, w.sorted_boxes, w.sorted_scores, ww.n);
  hipLaunchKernelGGL(nms_matrix_kernel, dim3((words + 3) / 4, words, nb), dim3(256), 0, s, w.sorted_boxes, ww.n, packed, words,
                     d->nms_thresh, ww.matrix);
  ScanOut o{d->out_boxes, d->out_scores, nullptr, nullptr, d->out_count, d->cap, nullptr, nullptr, 0, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(nms_scan_kernel, dim3(nb), dim3(1024), 0, s, w.sorted_boxes, w.sorted_scores, ww.n, packed, words, ww.matrix,
                     d->post_nms_topk, o);
  return eod_launch_status();
}

extern "C" int eod_centernet_proposals(const EodProposalDesc* d, eod_stream_t stream) {
  if (!d || !d->head_out || !d->out_boxes || !d->out_scores || !d->out_count || !d->workspace) return EOD_ERR_NULL;
  if (d->levels < 1 || d->levels > 5 || d->pre_nms_topk < 1 || d->head_stride < 5) return EOD_ERR_BAD_DIMS;
  const int slots = d->levels * d->pre_nms_topk;
  if (slots > 8192) return centernet_proposals_wide(d, (hipStream_t)stream);
  const int nb = d->batch > 1 ? d->batch : 1;
  CnArgs a{};
  if (const int err = cn_args(d, nb, &a)) return err;
  if (d->cap < d->post_nms_topk || d->cap > NMS_KEPT_MAX) return EOD_ERR_CAPACITY;
  if (nb > EOD_MAX_BATCH) return EOD_ERR_BAD_DIMS;
  const SelWs w = carve(d->workspace, slots * nb, slots, slots * nb);
  if (d->workspace_bytes < w.bytes) return EOD_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  cn_launch_level_topk(&a, w, s);
  ScanOut o{d->out_boxes, d->out_scores, nullptr, nullptr, d->out_count, d->cap, nullptr, nullptr, 0, nullptr, nullptr, nullptr};
  if (a.pk_off[d->levels] <= 4096)
    hipLaunchKernelGGL(cn_merge_nms_kernel<4>, dim3(nb), dim3(1024), 0, s, a, w.sorted_boxes, w.sorted_scores, d->nms_thresh,
                       d->post_nms_topk, o);
  else
    hipLaunchKernelGGL(cn_merge_nms_kernel<8>, dim3(nb), dim3(1024), 0, s, a, w.sorted_boxes, w.sorted_scores, d->nms_thresh,
                       d->post_nms_topk, o);
  return eod_launch_status();
}

// the wide path takes over beyond the single-workgroup kernel's classes or slots
static bool det_is_wide(int R_cap, int C1) { return C1 - 1 > DET_MAX_C || (long long)R_cap * (C1 - 1) > 8192; }

extern "C" size_t eod_detections_workspace_bytes(int R_cap, int C1) {
  if (R_cap <= 0 || R_cap > DET_MAX_R || C1 < 2 || C1 - 1 > DETW_MAX_C) return 0;
  if (det_is_wide(R_cap, C1)) return carve_detw(nullptr, C1 - 1, EOD_MAX_BATCH).bytes;
  const int slots = R_cap * (C1 - 1);
  return carve(nullptr, slots, slots, 0).bytes;
}

// the outputs of a detection call as the kernels take them; the optional lists need their counts (and the unique list a capacity)
static int det_outputs(const EodDetDesc* d, ScanOut* o) {
  if (d->out_unique_rows && (!d->out_unique_count || d->unique_cap <= 0)) return EOD_ERR_BAD_DIMS;
  if (d->out_rep_of && (!d->out_rep_list || !d->out_rep_count)) return EOD_ERR_BAD_DIMS;
  *o = ScanOut{d->out_boxes, d->out_scores, d->out_classes, d->out_rows, d->out_count, d->topk, d->out_unique_rows, d->out_unique_count,
               d->unique_cap, d->out_rep_of, d->out_rep_list, d->out_rep_count};
  return EOD_OK;
}

// EodDetDesc.row_matrix_out: the call is the matrix launch alone
static int det_build_row_matrix(const EodDetDesc* d, hipStream_t s) {
  if (!d->boxes) return EOD_ERR_NULL;
  const int nb = d->batch > 1 ? d->batch : 1;
  if (d->R_cap <= 0 || d->R_cap > DET_MAX_R || nb > EOD_MAX_BATCH) return EOD_ERR_BAD_DIMS;
  if ((uintptr_t)d->row_matrix_out & 7) return EOD_ERR_ALIGN;
  const int words = (d->R_cap + 63) >> 6;
  hipLaunchKernelGGL(det_row_matrix_kernel, dim3(words, words, nb), dim3(256), 0, s, d->boxes, d->count, d->R_cap, words, d->img_w,
                     d->img_h, d->nms_thresh, (u64*)d->row_matrix_out);
  return eod_launch_status();
}

extern "C" int eod_fast_rcnn_inference(const EodDetDesc* d, eod_stream_t stream) {
  if (d && d->row_matrix_out) return det_build_row_matrix(d, (hipStream_t)stream);
  if (!d || !d->boxes || !d->scores || !d->out_boxes || !d->out_scores || !d->out_classes || !d->out_rows || !d->out_count ||
      !d->workspace)
    return EOD_ERR_NULL;
  if (d->R_cap <= 0 || d->R_cap > DET_MAX_R || d->C1 < 2 || d->C1 - 1 > DETW_MAX_C || d->topk <= 0 || d->topk > NMS_KEPT_MAX)
    return EOD_ERR_BAD_DIMS;
  hipStream_t s = (hipStream_t)stream;
  const int nb = d->batch > 1 ? d->batch : 1;
  ScanOut o{};
  if (det_is_wide(d->R_cap, d->C1)) {
    if (nb > EOD_MAX_BATCH || d->row_matrix) return EOD_ERR_BAD_DIMS;      // the wide tail builds its matrix itself
    const DetwWs w = carve_detw(d->workspace, d->C1 - 1, EOD_MAX_BATCH);
    if (d->workspace_bytes < w.bytes) return EOD_ERR_CAPACITY;
    if (const int err = det_outputs(d, &o)) return err;
    if (!eod_aligned16(d->workspace)) return EOD_ERR_ALIGN;
    const dim3 grid((d->R_cap + 1) / 2, nb);
    hipLaunchKernelGGL(detw_hist_kernel, grid, dim3(256), 0, s, d->boxes, d->scores, d->count, d->R_cap, d->C1, d->score_thresh, w);
    hipLaunchKernelGGL(detw_compact_kernel, grid, dim3(256), 0, s, d->scores, d->count, d->R_cap, d->C1, d->score_thresh, w);
    hipLaunchKernelGGL(detw_tail_kernel, dim3(nb), dim3(1024), 0, s, d->boxes, d->scores, d->count, d->R_cap, d->C1, d->img_w, d->img_h,
                       d->score_thresh, d->nms_thresh, d->topk, w, o);
    return eod_launch_status();
  }
  const int slots = d->R_cap * (d->C1 - 1);
  const SelWs w = carve(d->workspace, slots, slots, 0);
  if (d->workspace_bytes < w.bytes) return EOD_ERR_CAPACITY;
  // (the single-workgroup kernel's row flags cover NMS_KEPT_MAX rows)
  if ((d->out_unique_rows || d->out_rep_of) && d->R_cap > NMS_KEPT_MAX) return EOD_ERR_BAD_DIMS;
  if (const int err = det_outputs(d, &o)) return err;
  if (nb > EOD_MAX_BATCH) return EOD_ERR_BAD_DIMS;
  if (d->row_matrix && ((uintptr_t)d->row_matrix & 7)) return EOD_ERR_ALIGN;
  hipLaunchKernelGGL(det_select_kernel, dim3(nb), dim3(1024), 0, s, d->boxes, d->scores, d->count, d->R_cap, d->C1, d->img_w, d->img_h,
                     d->score_thresh, d->nms_thresh, d->topk, o, (const u64*)d->row_matrix);
  return eod_launch_status();
}

extern "C" int eod_concat_lists(const int32_t* lists, const int32_t* counts, int cap_in, int id_stride, int batch, int32_t* out,
                                int32_t* out_count, eod_stream_t stream) {
  if (!lists || !counts || !out || !out_count) return EOD_ERR_NULL;
  if (cap_in <= 0 || id_stride <= 0 || batch < 1 || batch > EOD_MAX_BATCH) return EOD_ERR_BAD_DIMS;
  hipLaunchKernelGGL(concat_lists_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lists, counts, cap_in, id_stride, batch, out, out_count);
  return eod_launch_status();
}
