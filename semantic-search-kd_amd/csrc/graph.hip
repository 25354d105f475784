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
// Integer compares only.  The list of a neighbour comes from a look-up (KnnLists: the one k-NN table of a build;
// InsertLists: the adjacency of the rows already linked or the k-NN lists of the rows being inserted), so the build and
// the insertion run the same body.  graph_merge_kernel: one wave per row joins forward and reverse edges without
// duplicates; rows are numbered from row_base, so it serves a whole build and the slice of an insertion alike.
//
// graph_link_kernel (incremental insertion: sskd_graph_link), one workgroup of 256 threads per touched row u: the valid
// entries of graph[u] and of incoming[u] are packed without repeats (wave 0, two ballots), the first M / 2 of graph[u]
// stay, everything after them is the pool; row u is the query in LDS, the pool (at most M <= 64 rows) is staged as in
// row_stage.h in two chunks of 32, the second loading while wave 0 scores the first; the best M - |head| rows of the
// pool follow the head in rank order - each pool row counts the pool rows that rank before it (l_before: NaN after every
// number, then lower id, so the order is total and the places distinct).  A workgroup reads and writes its own row only,
// reads it whole before the barrier that precedes the first write, and writes every element of it once.
#include "ranking_walk.h"
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
    int total;
    const int mine = block_walk_pack<G_THREADS / 64>(open, lane, wave, wcount_s, total);
    if (total == 0) break;   // (uniform)
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

// entry e of a sequence of L candidate edges of row u is kept: a valid edge that no earlier entry names
__device__ inline bool g_first_edge(const int* seq, int e, int L, int u, int64_t n_rows) {
  if (e >= L || !g_edge_ok(seq[e], u, n_rows)) return false;
  for (int b = 0; b < e; ++b)
    if (seq[b] == seq[e]) return false;
  return true;
}

// Where graph_prune_kernel finds the list N(w) of a neighbour w (w is valid: in [0, n_total)) and how wide it is.
struct KnnLists {             // a build: every row's list is a row of the k-NN table
  const int32_t* knn;
  int K0;
  __device__ const int32_t* list(int w, int& width) const { width = K0; return knn + (int64_t)w * K0; }
};
struct InsertLists {          // an insertion: rows below n_old have their adjacency, the rows being inserted their k-NN lists
  const int32_t* graph_old;   // [n_old][M]
  const int32_t* knn_new;     // [n_total - n_old][K0]
  int64_t n_old;
  int M, K0;
  __device__ const int32_t* list(int w, int& width) const {
    if (w < n_old) { width = M; return graph_old + (int64_t)w * M; }
    width = K0;
    return knn_new + ((int64_t)w - n_old) * K0;
  }
};

// one workgroup of G_KNN_MAX threads per row; thread j owns L[j].  knn / fwd hold the rows [row_base, row_base + grid),
// ids are global: an entry is valid in [0, n_total) when it is not the row itself.
template <typename Lists>
__global__ __launch_bounds__(G_KNN_MAX) void graph_prune_kernel(Lists lists, const int32_t* __restrict__ knn, int64_t row_base,
                                                                int64_t n_total, int K0, int M, int32_t* __restrict__ fwd) {
  __shared__ int lu_s[G_KNN_MAX];
  __shared__ int lv_s[G_KNN_MAX];
  __shared__ int det_s[G_KNN_MAX];
  const int j = threadIdx.x;
  const int64_t r = blockIdx.x;                  // the row's place in knn / fwd
  const int u = (int)(row_base + r);             // its id
  const int mine = j < K0 ? knn[r * K0 + j] : -1;
  const bool valid = g_edge_ok(mine, u, n_total);
  lu_s[j] = mine;
  __syncthreads();
  int det = 0;
  for (int i = 0; i + 1 < K0; ++i) {
    const int v = lu_s[i];                       // (uniform)
    if (!g_edge_ok(v, u, n_total)) continue;
    int width;
    const int32_t* lv = lists.list(v, width);    // (uniform)
    lv_s[j] = j < width ? lv[j] : -1;            // past the list's width: -1, which no valid entry equals
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
  if (valid && rank < M) fwd[r * M + rank] = mine;
  if (j >= n_valid && j < M) fwd[r * M + j] = -1;
}

// one wave per row: first M/2 of fwd, then rev, then the rest of fwd, every row once, cut to M, -1 padded.  fwd / rev /
// graph hold the rows [row_base, row_base + n_rows); ids are global and valid in [0, n_total).
__global__ __launch_bounds__(G_MERGE_THREADS) void graph_merge_kernel(const int32_t* __restrict__ fwd, const int32_t* __restrict__ rev,
                                                                int64_t n_rows, int64_t row_base, int64_t n_total, int M,
                                                                int32_t* __restrict__ graph) {
  __shared__ int seq_s[G_MERGE_THREADS / 64][G_M_MAX + G_M_MAX / 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * (G_MERGE_THREADS / 64) + wave;
  if (u >= n_rows) return;   // (wave-uniform; no workgroup barrier below)
  const int id = (int)(row_base + u);
  const int h = M / 2, L = M + h;
  int* seq = seq_s[wave];
  for (int e = lane; e < L; e += 64)
    seq[e] = e < h ? fwd[u * M + e] : e < M ? rev[u * h + (e - h)] : fwd[u * M + (e - h)];
  wave_lds_sync();
  const bool k0 = g_first_edge(seq, lane, L, id, n_total), k1 = g_first_edge(seq, lane + 64, L, id, n_total);
  const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int n0 = __popcll(m0), pos0 = __popcll(m0 & lt), pos1 = n0 + __popcll(m1 & lt);
  if (k0 && pos0 < M) graph[u * M + pos0] = seq[lane];
  if (k1 && pos1 < M) graph[u * M + pos1] = seq[lane + 64];
  const int total = n0 + __popcll(m1);
  if (lane >= total && lane < M) graph[u * M + lane] = -1;
}

// ------------------------------------------------------------------------------------- linking into linked rows
constexpr int G_LINK_SEQ = G_M_MAX + G_M_MAX / 2;          // graph[u] followed by incoming[u]
static_assert(G_M_MAX <= 2 * STAGE_ROWS && G_LINK_SEQ <= 128, "the pool is two chunks; one wave packs the sequence in two ballots");

// rank order made total: a NaN score ranks after every number, and among NaNs the lower id comes first
__device__ inline bool l_before(float sa, int ia, float sb, int ib) {
  const bool na = sa != sa, nb = sb != sb;
  if (na || nb) return na == nb ? ia < ib : nb;
  return ranks_before(sa, ia, sb, ib);
}

struct LinkLds {
  float4 rows[STAGE_FLOAT4];   // the current chunk of the pool
  float4 q[CHUNKS];            // row u
  int seq[G_LINK_SEQ];         // graph[u], then incoming[u]
  int kept[G_LINK_SEQ];        // the valid entries of seq without repeats, in order: head, then the pool
  float score[G_M_MAX];        // of the pool
  int n_kept, n_head;
};

__global__ __launch_bounds__(G_THREADS) void graph_link_kernel(const float* __restrict__ rows, int32_t* graph, int64_t n_old,
                                                              int64_t n_total, int M, const int32_t* __restrict__ touched,
                                                              const int32_t* __restrict__ incoming) {
  __shared__ LinkLds lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t t = blockIdx.x;
  const int u = touched[t];
  // (uniform) in place: two workgroups must never own one row, which strictly ascending entries rule out
  if (u < 0 || u >= n_old || (t > 0 && touched[t - 1] >= u)) return;
  const float4* rows4 = reinterpret_cast<const float4*>(rows);
  const int h = M / 2, L = M + h;
  int32_t* mine = graph + (int64_t)u * M;
  if (tid < CHUNKS) lds.q[tid] = rows4[(int64_t)u * CHUNKS + tid];
  if (tid < L) lds.seq[tid] = tid < M ? mine[tid] : incoming[t * h + (tid - M)];
  __syncthreads();
  if (wave == 0) {
    const bool k0 = g_first_edge(lds.seq, lane, L, u, n_total), k1 = g_first_edge(lds.seq, lane + 64, L, u, n_total);
    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int n0 = __popcll(m0);
    if (k0) lds.kept[__popcll(m0 & lt)] = lds.seq[lane];
    if (k1) lds.kept[n0 + __popcll(m1 & lt)] = lds.seq[lane + 64];
    if (lane == 0) {
      const int n_adj = __popcll(M == 64 ? m0 : m0 & ((1ull << M) - 1ull));   // entries kept out of graph[u]: M <= 64
      lds.n_kept = n0 + __popcll(m1);
      lds.n_head = min(h, n_adj);
    }
  }
  __syncthreads();
  const int n_head = lds.n_head, P = lds.n_kept - n_head;   // (uniform) P <= M: at most M - h of graph[u] and h incoming
  const int* pool = lds.kept + n_head;

  RowStage stage;
  auto load_chunk = [&](int ch) {
    const int* ids = pool + ch * STAGE_ROWS;
    const int left = P - ch * STAGE_ROWS;
    stage.load(rows4, tid, [&](int row) { return row < left ? ids[row] : -1; });
  };
  const int n_chunks = (P + STAGE_ROWS - 1) / STAGE_ROWS;
  if (n_chunks > 0) {   // (uniform)
    load_chunk(0);
    stage.store(lds.rows, tid);
  }
  __syncthreads();
  for (int ch = 0; ch < n_chunks; ++ch) {
    const bool more = ch + 1 < n_chunks;
    if (more) load_chunk(ch + 1);   // in flight while wave 0 scores
    if (wave == 0 && lane < STAGE_ROWS) {
      const int j = ch * STAGE_ROWS + lane;
      if (j < P) lds.score[j] = stage_score(lds.rows, lane, lds.q);
    }
    __syncthreads();   // the chunk has been read
    if (more) stage.store(lds.rows, tid);
    __syncthreads();
  }
  // graph[u] was read whole before the barriers above; every element is written once below
  const int n_out = min(M, n_head + P);
  if (tid < n_head) mine[tid] = lds.kept[tid];
  if (tid < P) {
    const float s = lds.score[tid];
    const int id = pool[tid];
    int rank = 0;
    for (int e = 0; e < P; ++e) rank += l_before(lds.score[e], pool[e], s, id);
    if (n_head + rank < M) mine[n_head + rank] = id;
  }
  if (tid >= n_out && tid < M) mine[tid] = -1;
}

bool graph_degree_ok(int M) { return M >= 4 && M <= G_M_MAX && M % 2 == 0; }

bool graph_shape_ok(int nq, int k, int ef, int width, int M, int n_seeds) {
  return nq >= 1 && k >= 1 && k <= ef && ef <= G_EF_MAX && width >= 1 && width <= G_WIDTH_MAX && graph_degree_ok(M) &&
         n_seeds >= 1 && n_seeds <= G_EF_MAX;
}

// sskd_graph_merge and sskd_graph_merge_rows: one set of checks, one launch
int graph_merge_rows(const char* who, const int32_t* d_fwd, const int32_t* d_rev, int64_t n_rows, int64_t row_base,
                     int64_t n_total, int M, int32_t* d_graph, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "%s: n_rows < 0", who);
  SSKD_REQUIRE(row_base >= 0, "%s: row_base < 0", who);
  SSKD_REQUIRE(graph_degree_ok(M), "%s: M=%d must be even and in [4, %d]", who, M, G_M_MAX);
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS && n_total < sskd::MAX_SHARD_ROWS, "%s: shard too large for int32 row ids", who);
  SSKD_REQUIRE(row_base <= n_total && n_rows <= n_total - row_base, "%s: rows [row_base, row_base + n_rows) outside [0, n_total=%lld)",
               who, (long long)n_total);
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_fwd && d_rev && d_graph, "%s: null pointer", who);
  const int per_block = G_MERGE_THREADS / 64;
  hipLaunchKernelGGL(graph_merge_kernel, dim3((unsigned)sskd::ceil_div(n_rows, per_block)), dim3(G_MERGE_THREADS), 0,
                     sskd::as_stream(stream), d_fwd, d_rev, n_rows, row_base, n_total, M, d_graph);
  return sskd::check_launch("graph_merge_kernel");
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
  hipLaunchKernelGGL(graph_prune_kernel<KnnLists>, dim3((unsigned)n_rows), dim3(G_KNN_MAX), 0, sskd::as_stream(stream),
                     KnnLists{d_knn, knn_k}, d_knn, (int64_t)0, n_rows, knn_k, M, d_fwd);
  return sskd::check_launch("graph_prune_kernel");
}

int sskd_graph_insert_prune(const int32_t* d_graph_old, int64_t n_old, const int32_t* d_knn_new, int64_t n_new, int knn_k,
                            int M, int32_t* d_fwd_new, void* stream) {
  SSKD_REQUIRE(n_old >= 0, "graph_insert_prune: n_old < 0");
  SSKD_REQUIRE(n_new >= 0, "graph_insert_prune: n_new < 0");
  SSKD_REQUIRE(graph_degree_ok(M), "graph_insert_prune: M=%d must be even and in [4, %d]", M, G_M_MAX);
  SSKD_REQUIRE(knn_k >= M && knn_k <= G_KNN_MAX, "graph_insert_prune: knn_k=%d outside [M=%d, %d]", knn_k, M, G_KNN_MAX);
  SSKD_REQUIRE(n_old < sskd::MAX_SHARD_ROWS && n_new < sskd::MAX_SHARD_ROWS && n_old + n_new < sskd::MAX_SHARD_ROWS,
               "graph_insert_prune: shard too large for int32 row ids");
  if (n_new == 0) return SSKD_OK;
  SSKD_REQUIRE(d_knn_new && d_fwd_new && (n_old == 0 || d_graph_old), "graph_insert_prune: null pointer");
  hipLaunchKernelGGL(graph_prune_kernel<InsertLists>, dim3((unsigned)n_new), dim3(G_KNN_MAX), 0, sskd::as_stream(stream),
                     InsertLists{d_graph_old, d_knn_new, n_old, M, knn_k}, d_knn_new, n_old, n_old + n_new, knn_k, M, d_fwd_new);
  return sskd::check_launch("graph_insert_prune_kernel");
}

int sskd_graph_merge(const int32_t* d_fwd, const int32_t* d_rev, int64_t n_rows, int M, int32_t* d_graph, void* stream) {
  return graph_merge_rows("graph_merge", d_fwd, d_rev, n_rows, 0, n_rows, M, d_graph, stream);
}

int sskd_graph_merge_rows(const int32_t* d_fwd, const int32_t* d_incoming, int64_t n_rows, int64_t row_base, int64_t n_total,
                          int M, int32_t* d_graph_rows, void* stream) {
  return graph_merge_rows("graph_merge_rows", d_fwd, d_incoming, n_rows, row_base, n_total, M, d_graph_rows, stream);
}

int sskd_graph_link(const float* d_tiled, int32_t* d_graph, int64_t n_old, int64_t n_total, int M, const int32_t* d_touched,
                    const int32_t* d_incoming, int64_t n_touched, void* stream) {
  SSKD_REQUIRE(n_old >= 0, "graph_link: n_old < 0");
  SSKD_REQUIRE(n_total >= n_old, "graph_link: n_total=%lld < n_old=%lld", (long long)n_total, (long long)n_old);
  SSKD_REQUIRE(n_touched >= 0, "graph_link: n_touched < 0");
  SSKD_REQUIRE(graph_degree_ok(M), "graph_link: M=%d must be even and in [4, %d]", M, G_M_MAX);
  SSKD_REQUIRE(n_total < sskd::MAX_SHARD_ROWS, "graph_link: shard too large for int32 row ids");
  SSKD_REQUIRE(n_touched < sskd::MAX_SHARD_ROWS, "graph_link: n_touched too large");
  if (n_touched == 0) return SSKD_OK;
  SSKD_REQUIRE(d_tiled && d_graph && d_touched && d_incoming, "graph_link: null pointer");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0, "graph_link: the index must be 16-byte aligned");
  hipLaunchKernelGGL(graph_link_kernel, dim3((unsigned)n_touched), dim3(G_THREADS), 0, sskd::as_stream(stream), d_tiled,
                     d_graph, n_old, n_total, M, d_touched, d_incoming);
  return sskd::check_launch("graph_link_kernel");
}

}  // extern "C"
