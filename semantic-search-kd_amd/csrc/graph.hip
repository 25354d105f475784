// Graph index over the flat index (sskd_amd.h "Graph index"): a fixed-degree k-NN graph, beam search with exact scores.
//
// The reference's default index type is `hnsw` (configs/index.yaml:4-11: M 32, efConstruction 200, efSearch 64).  This
// file is a single-layer graph in its place: WHICH rows a query looks at is approximate (the rows a beam search over the
// graph reaches); every score and every order is exact - a row is scored by one lane running row_score_fma, the fma chain
// of the exact scan, and every list is kept in ranks_before order (score descending, then lower id).
//
// graph_search_kernel, one workgroup of 256 threads per query, everything it keeps in LDS:
//   T       the ef best rows scored so far, SORTED in rank order, whatever the mask says; bit 31 of an id = "expanded"
//   R       the k best ALLOWED rows scored so far, sorted (kept only when a mask is given: without one R is T's head)
//   cand    the rows offered in this step (the seeds, then the neighbours of up to `width` parents: at most 512)
//   seen    a hash table of row ids (full keys) that spares a row a second scoring
// A step = pick the first `width` unexpanded entries of T, gather their neighbours, drop ids outside the index and ids
// the table holds, score the rest in chunks of 32 rows, staged as in row_stage.h (all threads load the NEXT chunk into
// registers while wave 0 scores the CURRENT one out of LDS, one lane per row, as ivf_scan_kernel does), and merge
// the scores into T (and R).  The merge is a rank computation, not an insertion loop: a candidate's place in
// the new list is (entries of the old list that rank before it, by binary search) + (candidates that rank before it);
// an old entry's place is its index + (candidates that rank before it).  Places are distinct because the order is
// total and the candidates that take part are distinct rows none of which the list holds; whatever lands past the
// capacity is dropped.  The new list is written to the list's second buffer and the two swap.
//   Offering a row twice changes nothing: if the list still holds it the binary search lands on it (same id, same
// score bits) and it is dropped; if the list dropped it, the list's worst entry has only improved since and it ranks
// after it.  So `seen` is an optimisation only.  It may forget (a row whose 8 probe slots are taken is scored and not
// recorded; past 1 024 recorded rows the table is cleared and refilled with T), which costs a re-score.  It never
// reports a row it was not given: slots hold whole row ids, and a row is entered by the very lane that then offers it.
//   A NaN score never enters a list (g_merge drops it), so the order inside a list is total and every slot below
// `count` has been written; a query holding NaN therefore returns padding, without fault.
//   Every loop bound and every branch around a barrier is workgroup-uniform (read from LDS after a barrier, or a kernel
// argument), and the step loop ends after max_iterations at the latest.
//
// graph_prune_kernel: one workgroup per row u, thread j owns entry j of u's k-NN list and counts its detours in a
// register - for every i < j, whether the list of L_u[i] (staged in LDS) names L_u[j] among its first j entries.
// Integer compares only.  graph_merge_kernel: one wave per row joins forward and reverse edges without duplicates.
#include "row_stage.h"
#include "search_host.h"

#include <cfloat>

namespace {

constexpr int G_THREADS = STAGE_THREADS;                   // graph_search_kernel's workgroup is the staging workgroup
constexpr int G_MERGE_THREADS = 256;                       // graph_merge_kernel: four rows per workgroup, one wave each
constexpr int G_EF_MAX = 256;
constexpr int G_WIDTH_MAX = 8;
constexpr int G_M_MAX = 64;
constexpr int G_CAND = G_WIDTH_MAX * G_M_MAX;              // 512 rows offered in one step, at most
constexpr int G_SEEN = 2048;                               // slots of the visited table
constexpr int G_SEEN_PROBES = 8;
constexpr int G_SEEN_RESET = 1024;                         // recorded rows after which the table starts over
constexpr int G_KNN_MAX = 128;
constexpr int G_EXPANDED = (int)0x80000000;
constexpr int G_ID = 0x7FFFFFFF;
static_assert(G_CAND >= G_EF_MAX, "the seeds of a query fit the candidate buffer");

struct GraphParams {
  const float* rows;          // the index: row-major fp32 [n_rows][DIM]
  const int32_t* graph;       // [n_rows][M], -1 = no edge
  const float* queries;       // [nq][DIM], prepared
  const int64_t* seeds;       // [nq][n_seeds]
  const int32_t* seed_rows;   // null, or [n_seed_rows]: a seed s stands for row seed_rows[s]
  const uint32_t* row_mask;   // allow-mask words or null
  int64_t n_rows;
  int64_t n_seed_rows;
  int64_t id_offset;
  int M, n_seeds, k, ef, width, max_iterations;
  float* out_scores;          // [nq][k]
  int64_t* out_ids;
  int32_t* out_iterations;    // null or [nq]
};

// one sorted list (T or R): two buffers of G_EF_MAX entries each, `cur` says which one holds the list
struct GList {
  float* sbuf;
  int* ibuf;
  int cur, count, cap;
  __device__ float& s(int e) const { return sbuf[cur * G_EF_MAX + e]; }
  __device__ int& i(int e) const { return ibuf[cur * G_EF_MAX + e]; }
  __device__ float& s2(int e) const { return sbuf[(cur ^ 1) * G_EF_MAX + e]; }
  __device__ int& i2(int e) const { return ibuf[(cur ^ 1) * G_EF_MAX + e]; }
};

// the LDS of one workgroup of graph_search_kernel (sskd_graph_search_plan reports its size)
struct GraphLds {
  float4 rows[STAGE_FLOAT4];   // the current chunk
  float4 q[CHUNKS];
  float t_s[2 * G_EF_MAX];
  int t_i[2 * G_EF_MAX];
  float r_s[2 * G_EF_MAX];
  int r_i[2 * G_EF_MAX];
  float cand_s[G_CAND];
  int cand_i[G_CAND];
  int seen[G_SEEN];
  short place[G_CAND];
  int parent[G_WIDTH_MAX];
  int wcount[G_THREADS / 64];
  int cand_n, n_valid;
};
static_assert(2 * sizeof(GraphLds) <= 160 * 1024, "two workgroups per compute unit");

// entries of the list that rank before (s, id)
__device__ inline int g_lower(const GList& l, float s, int id) {
  int lo = 0, hi = l.count;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ranks_before(l.s(mid), l.i(mid) & G_ID, s, id)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ inline unsigned g_hash(int id) { return ((unsigned)id * 2654435761u) >> 21; }   // 11 bits: G_SEEN slots
static_assert(G_SEEN == 1 << 11, "g_hash returns a slot number");

// true when the table already holds `id`; otherwise the id is recorded if one of its probe slots is free
__device__ inline bool g_seen(int* seen, int id) {
  const unsigned h = g_hash(id);
#pragma unroll 1
  for (int p = 0; p < G_SEEN_PROBES; ++p) {
    const int old = atomicCAS(&seen[(h + p) & (G_SEEN - 1)], -1, id);
    if (old == -1) return false;
    if (old == id) return true;
  }
  return false;
}

// Merges the scored candidates cand_i / cand_s [0, C) into the list (see the head of the file).  `mask`: only rows whose
// bit is set take part (null: all).  place[] is scratch of G_CAND shorts; n_valid one LDS word.  Called by all threads.
__device__ inline void g_merge(GList& l, const int* cand_i, const float* cand_s, int C, const uint32_t* __restrict__ mask,
                               short* place, int* n_valid, int tid) {
  if (tid == 0) *n_valid = 0;
  __syncthreads();
  for (int j = tid; j < C; j += G_THREADS) {
    const int id = cand_i[j];
    int tb = -1;
    // a NaN score (a query or a row holding NaN) ranks nowhere - ranks_before is false both ways - and would break the
    // "places are distinct" argument below: such a candidate takes no part, so every score a list holds is ordered
    if (id >= 0 && cand_s[j] == cand_s[j] && row_allowed(mask, id)) {
      tb = g_lower(l, cand_s[j], id);
      if (tb >= l.cap || (tb < l.count && (l.i(tb) & G_ID) == id)) tb = -1;   // past the end, or the list holds the row
    }
    place[j] = (short)tb;
    if (tb >= 0) atomicAdd(n_valid, 1);
  }
  __syncthreads();
  const int nv = *n_valid;   // (uniform)
  if (nv == 0) return;
  // candidates that take part and rank before (s, id): C <= 512 LDS reads (broadcast: every lane reads entry j) for each
  // of the at most 2 candidates and 1 list entry a thread owns, and only in a step that changes the list
  auto before = [&](float s, int id) {
    int n = 0;
    for (int j = 0; j < C; ++j)
      if (place[j] >= 0 && ranks_before(cand_s[j], cand_i[j], s, id)) ++n;
    return n;
  };
  for (int j = tid; j < C; j += G_THREADS) {
    if (place[j] < 0) continue;
    const float s = cand_s[j];
    const int id = cand_i[j];
    const int pos = place[j] + before(s, id);
    if (pos < l.cap) { l.s2(pos) = s; l.i2(pos) = id; }
  }
  for (int e = tid; e < l.count; e += G_THREADS) {
    const float s = l.s(e);
    const int idf = l.i(e);
    const int pos = e + before(s, idf & G_ID);
    if (pos < l.cap) { l.s2(pos) = s; l.i2(pos) = idf; }
  }
  __syncthreads();
  l.cur ^= 1;
  l.count = min(l.cap, l.count + nv);
}

__global__ __launch_bounds__(G_THREADS) void graph_search_kernel(GraphParams p) {
  __shared__ GraphLds lds;
  float4* rows_s = lds.rows;
  float4* q_s = lds.q;
  float* cand_s = lds.cand_s;
  int* cand_i = lds.cand_i;
  int* seen_s = lds.seen;
  short* place_s = lds.place;
  int* parent_s = lds.parent;
  int* wcount_s = lds.wcount;
  int& cand_n = lds.cand_n;
  int& n_valid = lds.n_valid;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const float4* rows4 = reinterpret_cast<const float4*>(p.rows);
  if (tid < CHUNKS) q_s[tid] = reinterpret_cast<const float4*>(p.queries)[(int64_t)q * CHUNKS + tid];
  for (int e = tid; e < G_SEEN; e += G_THREADS) seen_s[e] = -1;
  if (tid == 0) cand_n = 0;
  __syncthreads();

  GList T{lds.t_s, lds.t_i, 0, 0, p.ef};
  GList R{lds.r_s, lds.r_i, 0, 0, p.k};
  int recorded = 0;   // an upper bound of the rows the table holds (uniform)

  // a row that was found for offering: inside the index and not seen -> the candidate buffer
  auto collect = [&](int64_t row) {
    if (row < 0 || row >= p.n_rows) return;
    if (g_seen(seen_s, (int)row)) return;
    cand_i[atomicAdd(&cand_n, 1)] = (int)row;   // at most n_seeds or width * M calls per step: <= G_CAND
  };

  // scores the candidates and merges them into T and R; leaves cand_n = 0.  Barriers inside: called by all threads.
  auto offer = [&]() {
    __syncthreads();
    const int C = cand_n;   // (uniform)
    recorded += C;
    if (C > 0) {
      // a row twice in one step (possible only when the table had no room for it): the later copy goes.  At most
      // C (C - 1) / 2 <= 130 816 compares over the workgroup, 1 022 LDS reads for the thread that owns the last two.
      for (int j = tid; j < C; j += G_THREADS) {
        const int id = cand_i[j];
        bool dup = false;
        for (int e = 0; e < j; ++e) dup |= cand_i[e] == id;
        if (dup) cand_i[j] = -1;   // (the first copy is never overwritten, so a racing reader still finds it)
      }
      __syncthreads();
      RowStage stage;
      auto load_chunk = [&](int ch) {
        const int* ids = cand_i + ch * STAGE_ROWS;
        const int left = C - ch * STAGE_ROWS;
        stage.load(rows4, tid, [&](int row) { return row < left ? ids[row] : -1; });
      };
      const int n_chunks = (C + STAGE_ROWS - 1) / STAGE_ROWS;
      load_chunk(0);
      stage.store(rows_s, tid);
      __syncthreads();
      for (int ch = 0; ch < n_chunks; ++ch) {
        const bool more = ch + 1 < n_chunks;
        if (more) load_chunk(ch + 1);   // in flight while wave 0 scores
        if (wave == 0 && lane < STAGE_ROWS) {
          const int j = ch * STAGE_ROWS + lane;
          if (j < C && cand_i[j] >= 0) cand_s[j] = stage_score(rows_s, lane, q_s);
        }
        __syncthreads();   // the chunk has been read
        if (more) stage.store(rows_s, tid);
        __syncthreads();
      }
      g_merge(T, cand_i, cand_s, C, nullptr, place_s, &n_valid, tid);
      if (p.row_mask) g_merge(R, cand_i, cand_s, C, p.row_mask, place_s, &n_valid, tid);
    }
    __syncthreads();
    if (tid == 0) cand_n = 0;
    __syncthreads();
  };

  // the seeds
  for (int e = tid; e < p.n_seeds; e += G_THREADS) {
    int64_t s = p.seeds[(int64_t)q * p.n_seeds + e];
    if (p.seed_rows) s = (s >= 0 && s < p.n_seed_rows) ? (int64_t)p.seed_rows[s] : -1;
    collect(s);
  }
  offer();

  int it = 0;
  for (; it < p.max_iterations; ++it) {
    if (recorded > G_SEEN_RESET) {   // (uniform) start the table over with the rows T holds
      for (int e = tid; e < G_SEEN; e += G_THREADS) seen_s[e] = -1;
      __syncthreads();
      if (tid < T.count) (void)g_seen(seen_s, T.i(tid) & G_ID);
      recorded = T.count;
      __syncthreads();
    }
    // the first `width` unexpanded entries of T become the parents
    const bool open = tid < T.count && (T.i(tid) & G_EXPANDED) == 0;
    const unsigned long long m = __ballot(open);
    if (lane == 0) wcount_s[wave] = __popcll(m);
    __syncthreads();
    int ahead = 0, total = 0;
#pragma unroll
    for (int w = 0; w < G_THREADS / 64; ++w) {
      if (w < wave) ahead += wcount_s[w];
      total += wcount_s[w];
    }
    if (total == 0) break;   // (uniform)
    const int mine = ahead + __popcll(m & ((1ull << lane) - 1ull));
    if (open && mine < p.width) {
      parent_s[mine] = T.i(tid);
      T.i(tid) |= G_EXPANDED;
    }
    __syncthreads();
    const int n_edges = min(total, p.width) * p.M;
    for (int e = tid; e < n_edges; e += G_THREADS) {
      const int par = e / p.M;
      const int from = parent_s[par];
      // T only ever receives range-checked rows; the check is repeated where the row number becomes an address
      if (from >= 0 && from < p.n_rows) collect(p.graph[(int64_t)from * p.M + (e - par * p.M)]);
    }
    offer();
  }

  const GList& out = p.row_mask ? R : T;
  for (int e = tid; e < p.k; e += G_THREADS) {
    const bool have = e < out.count;
    p.out_scores[(int64_t)q * p.k + e] = have ? out.s(e) : -FLT_MAX;
    p.out_ids[(int64_t)q * p.k + e] = have ? (int64_t)(out.i(e) & G_ID) + p.id_offset : -1;
  }
  if (p.out_iterations && tid == 0) p.out_iterations[q] = it;
}

// ---------------------------------------------------------------------------------------------- building the graph
__device__ inline bool g_edge_ok(int v, int u, int64_t n_rows) { return v >= 0 && v < n_rows && v != u; }

// one workgroup of G_KNN_MAX threads per row u; thread j owns L_u[j]
__global__ __launch_bounds__(G_KNN_MAX) void graph_prune_kernel(const int32_t* __restrict__ knn, int64_t n_rows, int K0, int M,
                                                                int32_t* __restrict__ fwd) {
  __shared__ int lu_s[G_KNN_MAX];
  __shared__ int lv_s[G_KNN_MAX];
  __shared__ int det_s[G_KNN_MAX];
  const int j = threadIdx.x;
  const int u = blockIdx.x;
  const int mine = j < K0 ? knn[(int64_t)u * K0 + j] : -1;
  const bool valid = g_edge_ok(mine, u, n_rows);
  lu_s[j] = mine;
  __syncthreads();
  int det = 0;
  for (int i = 0; i + 1 < K0; ++i) {
    const int v = lu_s[i];                       // (uniform)
    if (!g_edge_ok(v, u, n_rows)) continue;
    if (j < K0) lv_s[j] = knn[(int64_t)v * K0 + j];
    __syncthreads();
    if (valid && j > i) {
      bool found = false;
      for (int e = 0; e < j; ++e) found |= lv_s[e] == mine;
      det += found;
    }
    __syncthreads();
  }
  det_s[j] = valid ? det : -1;
  __syncthreads();
  // place of entry j among the valid ones by (detours, j); n_valid for the padding
  int rank = 0, n_valid = 0;
  for (int e = 0; e < K0; ++e) {
    const int d = det_s[e];
    if (d < 0) continue;
    ++n_valid;
    if (valid && (d < det || (d == det && e < j))) ++rank;
  }
  if (valid && rank < M) fwd[(int64_t)u * M + rank] = mine;
  if (j >= n_valid && j < M) fwd[(int64_t)u * M + j] = -1;
}

// one wave per row: first M/2 of fwd, then rev, then the rest of fwd, every row once, cut to M, -1 padded
__global__ __launch_bounds__(G_MERGE_THREADS) void graph_merge_kernel(const int32_t* __restrict__ fwd, const int32_t* __restrict__ rev,
                                                                int64_t n_rows, int M, int32_t* __restrict__ graph) {
  __shared__ int seq_s[G_MERGE_THREADS / 64][G_M_MAX + G_M_MAX / 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * (G_MERGE_THREADS / 64) + wave;
  if (u >= n_rows) return;   // (wave-uniform; no workgroup barrier below)
  const int h = M / 2, L = M + h;
  int* seq = seq_s[wave];
  for (int e = lane; e < L; e += 64)
    seq[e] = e < h ? fwd[u * M + e] : e < M ? rev[u * h + (e - h)] : fwd[u * M + (e - h)];
  wave_lds_sync();
  auto keep = [&](int e) {
    if (e >= L || !g_edge_ok(seq[e], (int)u, n_rows)) return false;
    for (int b = 0; b < e; ++b)
      if (seq[b] == seq[e]) return false;
    return true;
  };
  const bool k0 = keep(lane), k1 = keep(lane + 64);
  const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int n0 = __popcll(m0), pos0 = __popcll(m0 & lt), pos1 = n0 + __popcll(m1 & lt);
  if (k0 && pos0 < M) graph[u * M + pos0] = seq[lane];
  if (k1 && pos1 < M) graph[u * M + pos1] = seq[lane + 64];
  const int total = n0 + __popcll(m1);
  if (lane >= total && lane < M) graph[u * M + lane] = -1;
}

bool graph_degree_ok(int M) { return M >= 4 && M <= G_M_MAX && M % 2 == 0; }

bool graph_shape_ok(int nq, int k, int ef, int width, int M, int n_seeds) {
  return nq >= 1 && k >= 1 && k <= ef && ef <= G_EF_MAX && width >= 1 && width <= G_WIDTH_MAX && graph_degree_ok(M) &&
         n_seeds >= 1 && n_seeds <= G_EF_MAX;
}

}  // namespace

extern "C" {

int sskd_graph_search_plan(int nq, int k, int ef, int width, int M, int n_seeds, int* workgroups, int* threads,
                           int* lds_bytes, int* step_rows) {
  SSKD_REQUIRE(graph_shape_ok(nq, k, ef, width, M, n_seeds),
               "graph_search_plan: needs nq >= 1, 1 <= k <= ef <= %d, 1 <= width <= %d, M even in [4, %d], 1 <= n_seeds <= %d",
               G_EF_MAX, G_WIDTH_MAX, G_M_MAX, G_EF_MAX);
  if (workgroups) *workgroups = nq;
  if (threads) *threads = G_THREADS;
  if (step_rows) *step_rows = width * M;
  if (lds_bytes) *lds_bytes = (int)sizeof(GraphLds);
  return SSKD_OK;
}

size_t sskd_graph_search_workspace_bytes(int nq, int k, int ef, int width, int M, int n_seeds) {
  (void)nq; (void)k; (void)ef; (void)width; (void)M; (void)n_seeds;
  return 0;   // a query's whole state is in LDS
}

int sskd_graph_search(const float* d_tiled, int64_t n_rows, const int32_t* d_graph, int M, const float* d_queries, int nq,
                      const int64_t* d_seeds, int n_seeds, const int32_t* d_seed_rows, int64_t n_seed_rows, int k, int ef,
                      int width, int max_iterations, int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores,
                      int64_t* d_out_ids, int32_t* d_out_iterations, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "graph_search: n_rows < 0");
  SSKD_REQUIRE(nq >= 0, "graph_search: nq < 0");
  SSKD_REQUIRE(ef >= 1 && ef <= G_EF_MAX, "graph_search: ef=%d outside [1, %d]", ef, G_EF_MAX);
  SSKD_REQUIRE(k >= 1 && k <= ef, "graph_search: k=%d outside [1, ef=%d]", k, ef);
  SSKD_REQUIRE(graph_degree_ok(M), "graph_search: M=%d must be even and in [4, %d]", M, G_M_MAX);
  SSKD_REQUIRE(width >= 1 && width <= G_WIDTH_MAX, "graph_search: width=%d outside [1, %d]", width, G_WIDTH_MAX);
  SSKD_REQUIRE(max_iterations >= 1, "graph_search: max_iterations=%d < 1", max_iterations);
  SSKD_REQUIRE(n_seeds >= 1 && n_seeds <= G_EF_MAX, "graph_search: n_seeds=%d outside [1, %d]", n_seeds, G_EF_MAX);
  SSKD_REQUIRE(n_seed_rows >= 0, "graph_search: n_seed_rows < 0");
  SSKD_REQUIRE(id_offset >= 0, "graph_search: id_offset < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "graph_search: shard too large for int32 row ids");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_queries && d_seeds && d_out_scores && d_out_ids, "graph_search: null pointer");
  SSKD_REQUIRE(n_rows == 0 || (d_tiled && d_graph), "graph_search: null index");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_queries) % 16 == 0 && reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0,
               "graph_search: queries and index must be 16-byte aligned");
  GraphParams p{};
  p.rows = d_tiled;
  p.graph = d_graph;
  p.queries = d_queries;
  p.seeds = d_seeds;
  p.seed_rows = d_seed_rows;
  p.row_mask = d_row_mask;
  p.n_rows = n_rows;
  p.n_seed_rows = n_seed_rows;
  p.id_offset = id_offset;
  p.M = M;
  p.n_seeds = n_seeds;
  p.k = k;
  p.ef = ef;
  p.width = width;
  p.max_iterations = max_iterations;
  p.out_scores = d_out_scores;
  p.out_ids = d_out_ids;
  p.out_iterations = d_out_iterations;
  hipLaunchKernelGGL(graph_search_kernel, dim3((unsigned)nq), dim3(G_THREADS), 0, sskd::as_stream(stream), p);
  return sskd::check_launch("graph_search_kernel");
}

int sskd_graph_prune(const int32_t* d_knn, int64_t n_rows, int knn_k, int M, int32_t* d_fwd, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "graph_prune: n_rows < 0");
  SSKD_REQUIRE(graph_degree_ok(M), "graph_prune: M=%d must be even and in [4, %d]", M, G_M_MAX);
  SSKD_REQUIRE(knn_k >= M && knn_k <= G_KNN_MAX, "graph_prune: knn_k=%d outside [M=%d, %d]", knn_k, M, G_KNN_MAX);
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "graph_prune: shard too large for int32 row ids");
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_knn && d_fwd, "graph_prune: null pointer");
  hipLaunchKernelGGL(graph_prune_kernel, dim3((unsigned)n_rows), dim3(G_KNN_MAX), 0, sskd::as_stream(stream), d_knn, n_rows,
                     knn_k, M, d_fwd);
  return sskd::check_launch("graph_prune_kernel");
}

int sskd_graph_merge(const int32_t* d_fwd, const int32_t* d_rev, int64_t n_rows, int M, int32_t* d_graph, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "graph_merge: n_rows < 0");
  SSKD_REQUIRE(graph_degree_ok(M), "graph_merge: M=%d must be even and in [4, %d]", M, G_M_MAX);
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "graph_merge: shard too large for int32 row ids");
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_fwd && d_rev && d_graph, "graph_merge: null pointer");
  const int per_block = G_MERGE_THREADS / 64;
  hipLaunchKernelGGL(graph_merge_kernel, dim3((unsigned)sskd::ceil_div(n_rows, per_block)), dim3(G_MERGE_THREADS), 0,
                     sskd::as_stream(stream), d_fwd, d_rev, n_rows, M, d_graph);
  return sskd::check_launch("graph_merge_kernel");
}

}  // extern "C"
