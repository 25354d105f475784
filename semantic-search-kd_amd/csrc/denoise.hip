// Denoising of mined hard negatives (sskd_amd.h "Denoising of a ranking").
//
// The reference's rule (docs/guides/hyperparameter-tuning.md:107, configs/kd.yaml `denoising:`): a mined passage whose
// teacher score is >= 0.7 or whose text overlap with a positive is > 0.8 is a false negative and is dropped.  The
// overlap is the Jaccard similarity of the two texts' character 3-gram sets (src/utils/chunk.py:150-182).  Here a set
// is a strictly ascending list of uint64 keys in HBM (a CSR over the corpus rows, built by denoise.py), so
// |A n B| is a count of binary-search hits and the similarity is ONE fp64 division of two integers: the bits of
// Python's `int / int`.
//
//   rank_denoise_kernel   one workgroup of 256 threads per query.  For each positive in turn its key list is staged in
//                         LDS (at most 4 096 keys, 32 KiB; a longer list is searched where it lies); wave w takes the
//                         ranks w, w + 4, ..., its lanes stride over the candidate's keys (coalesced 8-byte loads) and
//                         search each in the positive's list; the hits are counted by ballot + popcount and the wave's
//                         Jaccard value raises the rank's running maximum, an fp64 word per rank in LDS.  After the
//                         last positive 256 ranks per round are decided and the survivors are packed in rank order by
//                         a ballot prefix over the four waves.
//   overlap_pairs_kernel  one wave per pair, the shorter list searched in the longer.
// Every loop bound and every branch around a barrier depends on the query alone (workgroup-uniform).  A set number is
// range-checked before it becomes an address; the store itself (limits, ascending keys) is trusted, as the BM25
// postings are.
#include "ranking_walk.h"
#include "search_host.h"

#include <cfloat>
#include <climits>

namespace {

constexpr int DN_THREADS = 256;
constexpr int DN_WAVES = DN_THREADS / 64;
constexpr int DN_LDS_KEYS = 4096;   // keys of a positive staged in LDS at most (32 KiB)

struct DenoiseParams {
  const int64_t* lims;          // [n_sets + 1] or null (overlap rule off)
  const uint64_t* grams;        // every set's keys, ascending within a set
  int64_t n_sets;
  const float* rank_scores;     // [nq][search_k]
  const int64_t* rank_ids;      // set numbers (local rows), -1 padded
  int search_k;
  const int64_t* pos_lims;      // [nq + 1]
  const int32_t* pos_rows;      // or null
  const float* aux;             // [nq][search_k] or null (teacher rule off)
  double aux_threshold;
  double overlap_threshold;
  float* out_scores;            // [nq][search_k]
  int64_t* out_ids;
  float* out_aux;               // or null
  int32_t* out_counts;          // [nq]
  double* out_overlap;          // [nq][search_k] or null, aligned with the INPUT ranks
  uint8_t* out_reason;          // likewise
};

// Is `key` in the ascending list[0 .. n), n >= 1?  A branch-free lower bound: the trip count depends on n alone, so the
// lanes of a wave (all searching the same list) never diverge.
__device__ __forceinline__ bool has_key(const uint64_t* list, int n, uint64_t key) {
  const uint64_t* b = list;
  int len = n;
  while (len > 1) {
    const int half = len >> 1;
    b += (b[half - 1] < key) ? half : 0;
    len -= half;
  }
  return *b == key;
}

// |keys n list| by one wave: the lanes stride over keys[0 .. n) and search list[0 .. m), m >= 1 (wave-uniform result)
__device__ __forceinline__ int wave_intersection(const uint64_t* keys, int n, const uint64_t* list, int m, int lane) {
  int inter = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    bool hit = false;
    if (i < n) hit = has_key(list, m, keys[i]);
    inter += __popcll(__ballot(hit));
  }
  return inter;
}

// one correctly rounded fp64 division of two integers (0.0 when either set is empty: then inter = 0)
__device__ __forceinline__ double jaccard_of(int inter, int na, int nb) {
  if (inter == 0) return 0.0;
  return (double)inter / (double)((int64_t)na + (int64_t)nb - (int64_t)inter);
}

__global__ __launch_bounds__(DN_THREADS) void rank_denoise_kernel(DenoiseParams p) {
  __shared__ uint64_t s_keys[DN_LDS_KEYS];
  __shared__ double s_ov[SSKD_K_MAX];
  __shared__ int s_len;
  __shared__ int s_kept[DN_WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int q = blockIdx.x;
  const int K = p.search_k;
  const float* rs = p.rank_scores + (int64_t)q * K;
  const int64_t* ri = p.rank_ids + (int64_t)q * K;

  // ---- the walk's length: the first id -1 ends it
  if (tid == 0) s_len = K;
  for (int r = tid; r < K; r += DN_THREADS) s_ov[r] = 0.0;
  __syncthreads();
  for (int r = tid; r < K; r += DN_THREADS)
    if (ri[r] == -1) atomicMin(&s_len, r);
  __syncthreads();
  const int len = s_len;   // (workgroup-uniform)

  // ---- overlap(rank) = max over the positives of jaccard(rank's set, positive's set)
  if (p.lims) {
    const int64_t lo = p.pos_lims[q];
    const int64_t end = p.pos_lims[q + 1];
    const int64_t hi = (p.pos_rows && end > lo) ? end : lo;
    for (int64_t j = lo; j < hi; ++j) {
      // (every thread reads the same words: the three `continue`s are workgroup-uniform)
      const int64_t pr = p.pos_rows[j];
      if (pr < 0 || pr >= p.n_sets) continue;   // the empty set
      const int64_t pl = p.lims[pr];
      const int pn = (int)(p.lims[pr + 1] - pl);
      if (pn <= 0) continue;
      const bool staged = pn <= DN_LDS_KEYS;
      __syncthreads();   // every wave is done with the list staged before
      if (staged)
        for (int i = tid; i < pn; i += DN_THREADS) s_keys[i] = p.grams[pl + i];
      __syncthreads();
      for (int r = wave; r < len; r += DN_WAVES) {
        const int64_t row = ri[r];   // (wave-uniform)
        if (row < 0 || row >= p.n_sets) continue;
        const int64_t cl = p.lims[row];
        const int cn = (int)(p.lims[row + 1] - cl);
        if (cn <= 0) continue;
        const int inter = staged ? wave_intersection(p.grams + cl, cn, s_keys, pn, lane)
                                 : wave_intersection(p.grams + cl, cn, p.grams + pl, pn, lane);
        const double jac = jaccard_of(inter, cn, pn);
        // rank r belongs to this wave alone (r % DN_WAVES == wave)
        if (lane == 0 && jac > s_ov[r]) s_ov[r] = jac;
      }
    }
  }
  __syncthreads();

  // ---- the decisions, 256 ranks per round; survivors packed in rank order
  float* os = p.out_scores + (int64_t)q * K;
  int64_t* oi = p.out_ids + (int64_t)q * K;
  float* oa = p.out_aux ? p.out_aux + (int64_t)q * K : nullptr;
  int count = 0;   // (workgroup-uniform) survivors so far
  for (int base = 0; base < K; base += DN_THREADS) {
    const int r = base + tid;
    const bool walked = r < len;
    double o = 0.0;
    float s = -FLT_MAX, a = __builtin_nanf("");
    int64_t id = -1;
    unsigned reason = 0;
    if (walked) {
      o = s_ov[r];
      s = rs[r];
      id = ri[r];
      if (p.lims && o > p.overlap_threshold) reason |= 1u;
      if (p.aux) {
        a = p.aux[(int64_t)q * K + r];
        if ((double)a >= p.aux_threshold) reason |= 2u;   // a NaN compares false: kept
      }
    }
    const bool keep = walked && reason == 0;
    int total;
    const int at = count + block_walk_pack<DN_WAVES>(keep, lane, wave, s_kept, total);   // <= r
    if (keep) {
      os[at] = s;
      oi[at] = id;
      if (oa) oa[at] = a;
    }
    if (r < K) {
      if (p.out_overlap) p.out_overlap[(int64_t)q * K + r] = o;
      if (p.out_reason) p.out_reason[(int64_t)q * K + r] = (uint8_t)reason;
    }
    count += total;
    __syncthreads();   // s_kept is rewritten in the next round
  }
  for (int i = count + tid; i < K; i += DN_THREADS) {
    os[i] = -FLT_MAX;
    oi[i] = -1;
    if (oa) oa[i] = __builtin_nanf("");
  }
  if (tid == 0) p.out_counts[q] = count;
}

struct PairParams {
  const int64_t* lims;
  const uint64_t* grams;
  int64_t n_sets;
  const int32_t* a;
  const int32_t* b;
  int64_t n_pairs;
  int32_t* inter;
  int32_t* uni;
  double* jaccard;
};

// One wave per pair; the kernel has no workgroup barrier.
__global__ __launch_bounds__(DN_THREADS) void overlap_pairs_kernel(PairParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * DN_WAVES + (threadIdx.x >> 6);
  if (i >= p.n_pairs) return;   // (wave-uniform)
  const int64_t ra = p.a[i], rb = p.b[i];
  int64_t la = 0, lb = 0;
  int na = 0, nb = 0;
  if (ra >= 0 && ra < p.n_sets) {
    la = p.lims[ra];
    na = (int)(p.lims[ra + 1] - la);
  }
  if (rb >= 0 && rb < p.n_sets) {
    lb = p.lims[rb];
    nb = (int)(p.lims[rb + 1] - lb);
  }
  int inter = 0;
  if (na > 0 && nb > 0)
    inter = na <= nb ? wave_intersection(p.grams + la, na, p.grams + lb, nb, lane)
                     : wave_intersection(p.grams + lb, nb, p.grams + la, na, lane);
  if (lane == 0) {
    p.inter[i] = inter;
    p.uni[i] = na + nb - inter;
    p.jaccard[i] = jaccard_of(inter, na, nb);
  }
}

}  // namespace

extern "C" {

int sskd_overlap_pairs(const int64_t* d_gram_lims, const uint64_t* d_grams, int64_t n_sets, const int32_t* d_a,
                       const int32_t* d_b, int64_t n_pairs, int32_t* d_inter, int32_t* d_union, double* d_jaccard,
                       void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_sets >= 0, "overlap_pairs: n_sets < 0");
  SSKD_REQUIRE(n_pairs >= 0, "overlap_pairs: n_pairs < 0");
  SSKD_REQUIRE(n_pairs <= (int64_t)INT_MAX * DN_WAVES, "overlap_pairs: n_pairs too large for one launch");
  if (n_pairs == 0) return SSKD_OK;
  SSKD_REQUIRE(d_gram_lims && d_grams, "overlap_pairs: null store");
  SSKD_REQUIRE(d_a && d_b && d_inter && d_union && d_jaccard, "overlap_pairs: null pointer");
  PairParams p{};
  p.lims = d_gram_lims;
  p.grams = d_grams;
  p.n_sets = n_sets;
  p.a = d_a;
  p.b = d_b;
  p.n_pairs = n_pairs;
  p.inter = d_inter;
  p.uni = d_union;
  p.jaccard = d_jaccard;
  hipLaunchKernelGGL(overlap_pairs_kernel, dim3((unsigned)sskd::ceil_div(n_pairs, DN_WAVES)), dim3(DN_THREADS), 0,
                     sskd::as_stream(stream), p);
  return sskd::check_launch("overlap_pairs_kernel");
}

int sskd_rank_denoise(const int64_t* d_gram_lims, const uint64_t* d_grams, int64_t n_sets, const float* d_rank_scores,
                      const int64_t* d_rank_ids, int nq, int search_k, const int64_t* d_pos_lims,
                      const int32_t* d_pos_rows, const float* d_aux, double aux_threshold, double overlap_threshold,
                      float* d_out_scores, int64_t* d_out_ids, float* d_out_aux, int32_t* d_out_counts,
                      double* d_out_overlap, uint8_t* d_out_reason, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_sets >= 0, "rank_denoise: n_sets < 0");
  SSKD_REQUIRE(nq >= 0, "rank_denoise: nq < 0");
  SSKD_REQUIRE(search_k >= 1, "rank_denoise: search_k=%d < 1", search_k);
  SSKD_REQUIRE(search_k <= SSKD_K_MAX, "rank_denoise: search_k=%d > %d", search_k, SSKD_K_MAX);
  SSKD_REQUIRE((d_gram_lims == nullptr) == (d_grams == nullptr),
               "rank_denoise: the store needs both of its pointers (limits and keys), or neither");
  SSKD_REQUIRE(!d_gram_lims || overlap_threshold == overlap_threshold, "rank_denoise: overlap_threshold is NaN");
  SSKD_REQUIRE(!d_aux || aux_threshold == aux_threshold, "rank_denoise: aux_threshold is NaN");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_rank_scores && d_rank_ids && d_pos_lims && d_out_scores && d_out_ids && d_out_counts,
               "rank_denoise: null pointer");
  DenoiseParams p{};
  p.lims = d_gram_lims;
  p.grams = d_grams;
  p.n_sets = n_sets;
  p.rank_scores = d_rank_scores;
  p.rank_ids = d_rank_ids;
  p.search_k = search_k;
  p.pos_lims = d_pos_lims;
  p.pos_rows = d_pos_rows;
  p.aux = d_aux;
  p.aux_threshold = aux_threshold;
  p.overlap_threshold = overlap_threshold;
  p.out_scores = d_out_scores;
  p.out_ids = d_out_ids;
  p.out_aux = d_out_aux;
  p.out_counts = d_out_counts;
  p.out_overlap = d_out_overlap;
  p.out_reason = d_out_reason;
  hipLaunchKernelGGL(rank_denoise_kernel, dim3((unsigned)nq), dim3(DN_THREADS), 0, sskd::as_stream(stream), p);
  return sskd::check_launch("rank_denoise_kernel");
}

}  // extern "C"
