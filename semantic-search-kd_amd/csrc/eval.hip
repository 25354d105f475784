// Retrieval evaluation on the device: nDCG / MRR / recall / precision per cutoff, and the discordant pairs behind
// Kendall's tau (sskd_amd.h "Retrieval evaluation").
//
// Implements the judge behind the reference's metrics (reference: src/utils/metrics.py ndcg_at_k / mrr_at_k /
// recall_at_k / precision_at_k / kendall_tau; src/kd/eval.py KDEvaluator) for ALL queries of a call at once.  One
// workgroup of 256 threads per query:
//   sskd_eval_judge   looks the rows of a ranking some search wrote up in the query's judgements (binary search)
//   sskd_eval_lists   scores (or reads the scores of) the query's own candidate list, ranks it in LDS by counting,
//                     and counts the pairs a second score list orders the other way
//   cutoff_metrics    (both) the per-cutoff arithmetic: fp64, every operation rounded once (this translation unit is
//                     compiled without contraction), the sums in the order np.sum adds a contiguous fp64 vector
#include "search_device.h"
#include "search_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int CUT_MAX = 8;       // cutoffs per call
constexpr int K_CUT_MAX = 256;   // largest cutoff: the discount table's length
constexpr int LIST_MAX = 1024;   // longest candidate list of sskd_eval_lists
constexpr int DIM_MAX = 2048;    // widest embedding sskd_eval_lists scores itself (the query lives in LDS)

struct Cutoffs {
  int n;
  int k[CUT_MAX];   // strictly increasing, 1 .. K_CUT_MAX
};

// ---- np.sum over a contiguous fp64 vector (NumPy's pairwise_sum, block size 128, eight accumulators)
// m <= 128: fewer than 8 terms are added left to right from 0.0; otherwise r[j] = a[j], r[j] += a[i + j] for i = 8, 16,
// ... while i + 8 <= m, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail left to right
__device__ inline double np_sum_block(const double* a, int m) {
  if (m < 8) {
    double res = 0.0;
    for (int i = 0; i < m; ++i) res = res + a[i];
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i + 8 <= m; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < m; ++i) res = res + a[i];
  return res;
}
// m > 128 splits at h = m/2 - (m/2) % 8 and adds the two halves, each summed by the same rule.  For m <= 256 the second
// half can exceed 128 by up to 7 (m = 255: 120 + 135) and splits once more; its halves cannot.
__device__ inline double np_sum_once_split(const double* a, int m) {
  if (m <= 128) return np_sum_block(a, m);
  int h = m / 2;
  h -= h % 8;
  return np_sum_block(a, h) + np_sum_block(a + h, m - h);
}
__device__ inline double np_sum(const double* a, int m) {   // m <= 256
  if (m <= 128) return np_sum_block(a, m);
  int h = m / 2;
  h -= h % 8;
  return np_sum_once_split(a, h) + np_sum_once_split(a + h, m - h);
}

// descending order of grades for the ideal ranking: higher grade first, then lower position (positions are distinct)
__device__ inline bool grade_before(int32_t ga, int64_t ia, int32_t gb, int64_t ib) {
  return ga > gb || (ga == gb && ia < ib);
}

// LDS the per-cutoff arithmetic works in
struct MetricsLds {
  double terms[1 + CUT_MAX][K_CUT_MAX];   // row 0: g[i] / disc[i]; row 1 + c: the ideal list's terms of cutoff c
  double sums[2][CUT_MAX];                // DCG, IDCG
  int n_relevant;
};

// The per-cutoff metrics of one query (every thread of the workgroup calls it; `g` is complete and visible).
//   g         LDS: the grades in rank order, entries [0, min(n_ranked, 256))
//   judged    the query's judged grades (global, any order) and their number: n_relevant, and the ideal list of mode 1
//   out       [cut.n][4] = (ndcg, mrr, recall, precision)
__device__ void cutoff_metrics(const Cutoffs& cut, const int32_t* g, int n_ranked, const int32_t* __restrict__ judged,
                               int64_t n_judged, const double* __restrict__ disc, int ideal_mode, MetricsLds& L,
                               double* __restrict__ out) {
  const int tid = threadIdx.x;
  if (tid == 0) L.n_relevant = 0;
  __syncthreads();

  // ---- n_relevant
  int pos = 0;
  for (int64_t j = tid; j < n_judged; j += THREADS) pos += judged[j] > 0 ? 1 : 0;
  pos = wave_sum(pos);
  if ((tid & 63) == 0 && pos) atomicAdd(&L.n_relevant, pos);

  // ---- DCG terms: the cutoffs share them, cutoff c sums the first m_c
  const int m_last = min(cut.k[cut.n - 1], n_ranked);
  const int32_t mine = tid < m_last ? g[tid] : 0;
  if (tid < m_last) L.terms[0][tid] = (double)mine / disc[tid];

  // ---- ideal terms
  if (ideal_mode == 0) {
    // cutoff c: the first m_c retrieved grades in descending order.  One walk over the ranked list: when it has passed m_c
    // entries, `place` is where this thread's grade stands among them.
    int place = 0, j = 0;
    for (int c = 0; c < cut.n; ++c) {
      const int m = min(cut.k[c], n_ranked);
      for (; j < m; ++j) place += grade_before(g[j], j, mine, tid) ? 1 : 0;   // (the lanes read one entry: broadcast)
      if (tid < m) L.terms[1 + c][place] = (double)mine / disc[place];
    }
  } else {
    // every cutoff: a prefix of ALL judged grades in descending order; only the first 256 places can be asked for
    for (int64_t base = 0; base < n_judged; base += 4 * THREADS) {
      int32_t ge[4];
      int64_t ie[4];
      int64_t place[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ie[e] = base + tid + e * THREADS;
        ge[e] = ie[e] < n_judged ? judged[ie[e]] : 0;
      }
      for (int64_t jj = 0; jj < n_judged; ++jj) {
        const int32_t gj = judged[jj];   // (one address for the workgroup)
#pragma unroll
        for (int e = 0; e < 4; ++e) place[e] += grade_before(gj, jj, ge[e], ie[e]) ? 1 : 0;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ie[e] < n_judged && place[e] < K_CUT_MAX) L.terms[1][place[e]] = (double)ge[e] / disc[place[e]];
    }
  }
  __syncthreads();

  // ---- the sums: thread c adds DCG of cutoff c, thread 8 + c its IDCG
  if (tid < 2 * CUT_MAX) {
    const int c = tid & (CUT_MAX - 1), ideal = tid >> 3;
    if (c < cut.n) {
      const int m = min(cut.k[c], n_ranked);
      double s;
      if (!ideal) s = np_sum(L.terms[0], m);
      else if (ideal_mode == 0) s = np_sum(L.terms[1 + c], m);
      else s = np_sum(L.terms[1], (int)min((int64_t)cut.k[c], n_judged));
      L.sums[ideal][c] = s;
    }
  }
  __syncthreads();

  if (tid < cut.n) {
    const int k = cut.k[tid];
    const int m = min(k, n_ranked);
    int hits = 0, first = -1;
    for (int i = 0; i < m; ++i) {
      if (g[i] > 0) {
        ++hits;
        if (first < 0) first = i;
      }
    }
    const double dcg = L.sums[0][tid], idcg = L.sums[1][tid];
    double ndcg = 0.0, mrr = 0.0, recall = 0.0;
    if (idcg != 0.0) ndcg = dcg / idcg;
    if (first >= 0) mrr = 1.0 / (double)(first + 1);
    if (L.n_relevant > 0) recall = (double)hits / (double)L.n_relevant;
    const double precision = (double)hits / (double)k;
    double* o = out + 4 * tid;
    o[0] = ndcg;
    o[1] = mrr;
    o[2] = recall;
    o[3] = precision;
  }
}

__device__ inline void write_nan_metrics(const Cutoffs& cut, double* out) {
  for (int i = threadIdx.x; i < 4 * cut.n; i += THREADS) out[i] = __builtin_nan("");
}

// ------------------------------------------------------------------------- //
// sskd_eval_judge
// ------------------------------------------------------------------------- //
struct JudgeParams {
  const int64_t* rank_ids;     // [nq][k_rank]
  const int64_t* rel_lims;     // [nq + 1]
  const int32_t* rel_rows;     // ascending within a query; null: nothing is judged
  const int32_t* rel_grades;
  const double* disc;          // [256]
  double* out;                 // [nq][n_cut][4]
  int64_t n_rel;
  int64_t id_offset;
  int k_rank;
  int ideal_mode;
  Cutoffs cut;
};

__global__ __launch_bounds__(THREADS) void eval_judge_kernel(JudgeParams p) {
  __shared__ MetricsLds L;
  __shared__ int32_t g[K_CUT_MAX];
  __shared__ int first_pad;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  double* out = p.out + q * p.cut.n * 4;

  int64_t lo = 0, hi = 0;
  if (p.rel_rows) {
    lo = p.rel_lims[q];
    hi = p.rel_lims[q + 1];
    if (lo < 0 || hi < lo || hi > p.n_rel) {   // (uniform) limits that do not describe a slice of the judgements
      write_nan_metrics(p.cut, out);
      return;
    }
  }
  // only the first 256 places of a ranking can reach a cutoff
  const int walk = min(p.k_rank, K_CUT_MAX);
  if (tid == 0) first_pad = walk;
  __syncthreads();
  const int64_t id = tid < walk ? p.rank_ids[q * p.k_rank + tid] : 0;
  if (tid < walk && id == -1) atomicMin(&first_pad, tid);
  __syncthreads();
  const int n_ranked = first_pad;

  int32_t grade = 0;
  if (tid < n_ranked) {
    const int64_t row = id - p.id_offset;
    int64_t a = lo, b = hi;
    while (a < b) {
      const int64_t mid = a + ((b - a) >> 1);
      if ((int64_t)p.rel_rows[mid] < row) a = mid + 1;
      else b = mid;
    }
    if (a < hi && (int64_t)p.rel_rows[a] == row) grade = p.rel_grades[a];
  }
  g[tid] = grade;
  __syncthreads();
  cutoff_metrics(p.cut, g, n_ranked, p.rel_rows ? p.rel_grades + lo : nullptr, hi - lo, p.disc, p.ideal_mode, L, out);
}

// ------------------------------------------------------------------------- //
// sskd_eval_lists
// ------------------------------------------------------------------------- //
struct ListsParams {
  const float* queries;        // [nq][dim] or null
  const float* docs;           // [total][dim] or null
  const float* scores_in;      // [total] or null
  const int64_t* doc_lims;     // [nq + 1]
  const int32_t* grades;       // [total]
  const float* ref_scores;     // [total] or null
  const double* disc;          // [256]
  double* out;                 // [nq][n_cut][4]
  float* out_scores;           // [total] or null
  int32_t* out_order;          // [total] or null
  int64_t* out_discordant;     // [nq], written when ref_scores is given
  int64_t total;
  int dim;
  int ideal_mode;
  Cutoffs cut;
};

// strict "a ranks before b" within one list: ranks_before on the numbers (score descending, then lower position); a NaN
// ranks after every number, NaNs among themselves by position
__device__ inline bool list_before(float sa, int ia, float sb, int ib) {
  const bool na = sa != sa, nb = sb != sb;
  if (na || nb) return na == nb ? ia < ib : nb;
  return ranks_before(sa, ia, sb, ib);
}

// rank[e] of the thread's entries tid + 256 e under list_before: the number of entries that rank before it
__device__ inline void count_ranks(const float* s, int n, int (&rank)[4]) {
  const int tid = threadIdx.x;
  float se[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = tid + e * THREADS;
    se[e] = i < n ? s[i] : 0.f;
    rank[e] = 0;
  }
  for (int j = 0; j < n; ++j) {
    const float sj = s[j];   // (the lanes read one entry: broadcast)
#pragma unroll
    for (int e = 0; e < 4; ++e) rank[e] += list_before(sj, j, se[e], tid + e * THREADS) ? 1 : 0;
  }
}

__global__ __launch_bounds__(THREADS) void eval_lists_kernel(ListsParams p) {
  __shared__ MetricsLds L;
  __shared__ float4 q4[DIM_MAX / 4];
  __shared__ float s[LIST_MAX];
  __shared__ int32_t both[LIST_MAX];   // rank under the scores << 16 | rank under the reference scores
  __shared__ int32_t g[K_CUT_MAX];
  __shared__ int discordant;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  double* out = p.out + q * p.cut.n * 4;

  const int64_t lo = p.doc_lims[q], hi = p.doc_lims[q + 1];
  if (lo < 0 || hi < lo || hi > p.total || hi - lo > LIST_MAX) {   // (uniform) not a list this kernel may touch
    write_nan_metrics(p.cut, out);
    return;
  }
  const int n = (int)(hi - lo);

  // ---- scores
  if (p.scores_in) {
    for (int i = tid; i < n; i += THREADS) s[i] = p.scores_in[lo + i];
  } else {
    const int chunks = p.dim / 4;
    const float4* src = reinterpret_cast<const float4*>(p.queries) + q * chunks;
    for (int i = tid; i < chunks; i += THREADS) q4[i] = src[i];
    __syncthreads();
    for (int i = tid; i < n; i += THREADS)
      s[i] = row_score_fma(reinterpret_cast<const float4*>(p.docs) + (lo + i) * chunks,
                           reinterpret_cast<const float*>(q4), p.dim / 8);
  }
  if (p.out_scores)
    for (int i = tid; i < n; i += THREADS) p.out_scores[lo + i] = s[i];   // (each thread reads back what it wrote)
  if (tid == 0) discordant = 0;
  g[tid] = 0;
  __syncthreads();

  // ---- rank: the places are distinct, so the ranks are a permutation of 0 .. n - 1
  int rank[4];
  count_ranks(s, n, rank);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = tid + e * THREADS;
    if (i >= n) continue;
    if (p.out_order) p.out_order[lo + rank[e]] = i;
    if (rank[e] < K_CUT_MAX) g[rank[e]] = p.grades[lo + i];
  }

  // ---- discordant pairs against the reference scores, ranked by the same rule
  if (p.ref_scores) {
    __syncthreads();   // every thread is done reading s
    for (int i = tid; i < n; i += THREADS) s[i] = p.ref_scores[lo + i];
    __syncthreads();
    int ref_rank[4];
    count_ranks(s, n, ref_rank);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = tid + e * THREADS;
      if (i < n) both[i] = (rank[e] << 16) | ref_rank[e];
    }
    __syncthreads();
    int count = 0;
    for (int j = 0; j < n; ++j) {
      const int bj = both[j];   // (broadcast)
      const int aj = bj >> 16, rj = bj & 0xffff;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = tid + e * THREADS;
        // each unordered pair once (i < j; entries past n never count)
        count += (i < j && ((aj < rank[e]) != (rj < ref_rank[e]))) ? 1 : 0;
      }
    }
    count = wave_sum(count);
    if ((tid & 63) == 0 && count) atomicAdd(&discordant, count);   // at most 1024 * 1023 / 2
  }
  __syncthreads();
  if (p.ref_scores && tid == 0) p.out_discordant[q] = discordant;

  cutoff_metrics(p.cut, g, n, p.grades + lo, n, p.disc, p.ideal_mode, L, out);
}

// the checks both entry points share; fills `cut`
int check_common(const char* what, int nq, const int32_t* cutoffs, int n_cut, int ideal_mode, Cutoffs* cut) {
  SSKD_REQUIRE(nq >= 0, "%s: nq < 0", what);
  SSKD_REQUIRE(n_cut >= 1 && n_cut <= CUT_MAX, "%s: n_cut=%d outside [1, %d]", what, n_cut, CUT_MAX);
  SSKD_REQUIRE(cutoffs, "%s: null cutoffs", what);
  for (int c = 0; c < n_cut; ++c) {
    SSKD_REQUIRE(cutoffs[c] >= 1 && cutoffs[c] <= K_CUT_MAX, "%s: cutoff %d outside [1, %d]", what, cutoffs[c], K_CUT_MAX);
    SSKD_REQUIRE(c == 0 || cutoffs[c] > cutoffs[c - 1], "%s: the cutoffs must increase strictly", what);
    cut->k[c] = cutoffs[c];
  }
  cut->n = n_cut;
  SSKD_REQUIRE(ideal_mode == 0 || ideal_mode == 1, "%s: ideal_mode=%d is neither 0 (retrieved) nor 1 (judged)", what,
               ideal_mode);
  return SSKD_OK;
}

inline bool aligned_to(const void* ptr, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(ptr) % bytes == 0; }

}  // namespace

extern "C" {

int sskd_eval_judge(const int64_t* d_rank_ids, int nq, int k_rank, int64_t id_offset, const int64_t* d_rel_lims,
                    const int32_t* d_rel_rows, const int32_t* d_rel_grades, int64_t n_rel, const double* d_discounts,
                    const int32_t* cutoffs, int n_cut, int ideal_mode, double* d_out_metrics, void* stream) {
  // every check comes before the first HIP call
  JudgeParams p{};
  if (int rc = check_common("eval_judge", nq, cutoffs, n_cut, ideal_mode, &p.cut)) return rc;
  SSKD_REQUIRE(k_rank >= 1 && k_rank <= SSKD_K_MAX, "eval_judge: k_rank=%d outside [1, %d]", k_rank, SSKD_K_MAX);
  SSKD_REQUIRE(n_rel >= 0, "eval_judge: n_rel < 0");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_rank_ids && d_discounts && d_out_metrics, "eval_judge: null ranking, discount table or output");
  SSKD_REQUIRE(!d_rel_rows || (d_rel_lims && d_rel_grades), "eval_judge: d_rel_rows needs d_rel_lims and d_rel_grades");
  SSKD_REQUIRE(aligned_to(d_rank_ids, 8) && aligned_to(d_rel_lims, 8) && aligned_to(d_discounts, 8) &&
                   aligned_to(d_out_metrics, 8) && aligned_to(d_rel_rows, 4) && aligned_to(d_rel_grades, 4),
               "eval_judge: a pointer is not aligned to its element size");
  p.rank_ids = d_rank_ids;
  p.rel_lims = d_rel_lims;
  p.rel_rows = d_rel_rows;
  p.rel_grades = d_rel_grades;
  p.disc = d_discounts;
  p.out = d_out_metrics;
  p.n_rel = n_rel;
  p.id_offset = id_offset;
  p.k_rank = k_rank;
  p.ideal_mode = ideal_mode;
  hipLaunchKernelGGL(eval_judge_kernel, dim3((unsigned)nq), dim3(THREADS), 0, sskd::as_stream(stream), p);
  return sskd::check_launch("eval_judge_kernel");
}

int sskd_eval_lists(const float* d_queries, const float* d_docs, int dim, const float* d_scores_in,
                    const int64_t* d_doc_lims, int64_t total, const int32_t* d_grades, const float* d_ref_scores,
                    const double* d_discounts, const int32_t* cutoffs, int n_cut, int ideal_mode, int nq,
                    double* d_out_metrics, float* d_out_scores, int32_t* d_out_order, int64_t* d_out_discordant,
                    void* stream) {
  // every check comes before the first HIP call
  ListsParams p{};
  if (int rc = check_common("eval_lists", nq, cutoffs, n_cut, ideal_mode, &p.cut)) return rc;
  SSKD_REQUIRE(total >= 0, "eval_lists: total < 0");
  if (nq == 0) return SSKD_OK;
  if (!d_scores_in) {
    SSKD_REQUIRE(dim >= 8 && dim <= DIM_MAX && dim % 8 == 0, "eval_lists: dim=%d must be a multiple of 8 in [8, %d]", dim,
                 DIM_MAX);
    SSKD_REQUIRE(aligned_to(d_queries, 16) && aligned_to(d_docs, 16),
                 "eval_lists: d_queries and d_docs must be 16-byte aligned");
    SSKD_REQUIRE(d_queries && (d_docs || total == 0), "eval_lists: without d_scores_in, d_queries and d_docs are needed");
  }
  SSKD_REQUIRE(d_doc_lims && d_discounts && d_out_metrics, "eval_lists: null list limits, discount table or output");
  SSKD_REQUIRE(d_grades || total == 0, "eval_lists: null grades");
  SSKD_REQUIRE(!d_ref_scores || d_out_discordant, "eval_lists: d_ref_scores needs d_out_discordant");
  SSKD_REQUIRE(aligned_to(d_doc_lims, 8) && aligned_to(d_discounts, 8) && aligned_to(d_out_metrics, 8) &&
                   aligned_to(d_out_discordant, 8) && aligned_to(d_scores_in, 4) && aligned_to(d_ref_scores, 4) &&
                   aligned_to(d_grades, 4) && aligned_to(d_out_scores, 4) && aligned_to(d_out_order, 4),
               "eval_lists: a pointer is not aligned to its element size");
  p.queries = d_queries;
  p.docs = d_docs;
  p.scores_in = d_scores_in;
  p.doc_lims = d_doc_lims;
  p.grades = d_grades;
  p.ref_scores = d_ref_scores;
  p.disc = d_discounts;
  p.out = d_out_metrics;
  p.out_scores = d_out_scores;
  p.out_order = d_out_order;
  p.out_discordant = d_out_discordant;
  p.total = total;
  p.dim = dim;
  p.ideal_mode = ideal_mode;
  hipLaunchKernelGGL(eval_lists_kernel, dim3((unsigned)nq), dim3(THREADS), 0, sskd::as_stream(stream), p);
  return sskd::check_launch("eval_lists_kernel");
}

}  // extern "C"
